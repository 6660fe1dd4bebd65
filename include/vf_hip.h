/* vf_hip.h - C ABI of libvf_hip.so, the MI355X (gfx950) video-prediction + cost engine.
 *
 * The reference (SudeepDasari/visual_foresight) has no FFI: its planner crosses to the device
 * through one Python call into a TensorFlow-1 session.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  All bulk pointers
 * are DEVICE pointers owned by the caller (PyTorch-ROCm tensors are the usual carrier); small
 * control data (config, goal pixels) is passed by value / host pointer.  Every function
 * returns 0 on success or a negative vf_status; vf_last_error() describes the last failure of
 * the calling thread.  No exception crosses this boundary.  Every device buffer - packed
 * weights, activations, predictions, schedules - is sized from the config and allocated in
 * vf_create(); no later call allocates device memory (vf_load_weights refills the same
 * buffers).  vf_set_context / vf_rollout / vf_export / vf_register(_hw) / vf_resize_area / vf_cem_refit / vf_cem_sample / vf_cem_soft_refit / vf_cem_sample_corr / vf_cem_sample_fold / vf_cem_sample_autograsp / vf_cem_latents / vf_cem_fold_latents / vf_allgather_scores only
 * enqueue work on the caller's HIP stream (hipStream_t passed as void*; NULL = the default
 * stream) and never synchronise it; a handle is driven from one stream at a time.
 * vf_load_weights, vf_device_status and the debug hooks are the blocking calls.
 *
 * Tensor layouts (C order, float32 unless noted; ncam = views, the reference stacks views on
 * a camera axis, visual_mpc/video_prediction/vpred_model_interface.py:78,88):
 *   context frames   uint8  [n_context][ncam][H][W][3]
 *   context distrib         [n_context][ncam][H][W][ndesig]
 *   context states          [n_context][sdim]
 *   context actions         [n_context-1][adim]
 *   actions                 [B][T][adim]                    T = sequence_length - n_context
 *   predicted frames        [B][T][ncam][H][W][3]           in [0,1]
 *   predicted distrib       [B][T][ncam][H][W][ndesig]      each (b,t,c,.,.,p) plane sums to 1
 *   predicted states        [B][T][sdim]
 *   scores        float64   [B / n_draws], scores_per_task [B / n_draws][ncam * ndesig]
 *                           (camera-major, as pixel_cost_controller.py:138-149 stacks them; float64
 *                           like the reference's host cost under NumPy >= 2, so device rounding
 *                           cannot create ties in front of the elite argsort)
 */
#ifndef VF_HIP_H
#define VF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VF_ABI_VERSION 7

typedef enum vf_status {
    VF_OK = 0,
    VF_ERR_INVALID = -1,   /* bad argument / shape / state */
    VF_ERR_HIP = -2,       /* a HIP runtime call failed */
    VF_ERR_NOMEM = -3,     /* device allocation failed */
    VF_ERR_NOWEIGHTS = -4, /* rollout before vf_load_weights */
    VF_ERR_NOCONTEXT = -5  /* rollout before vf_set_context */
} vf_status;

/* Static shape of one predictor instance.  Replaces the `conf` dict + placeholders of
 * visual_mpc/video_prediction/setup_predictor.py:98-114 (orig_size, adim, sdim, ndesig,
 * context_frames, sequence_length, batch_size) and the predictor hparams of
 * visual_mpc/policy/cem_controllers/pixel_cost_controller.py:29-33
 * (designated_pixel_count, run_batch_size). */
typedef struct vf_config {
    int32_t height, width;      /* multiples of 8 */
    int32_t adim, sdim;
    int32_t ndesig;             /* designated pixels per view (0..4).  0 = a FRAMES-ONLY engine (arch 0 - 2; arch 3 refuses
                                 * it): the same frames and states, bit for bit, and no pixel distribution anywhere - none
                                 * allocated, staged, warped, summed, scored or exported (the reference's predictor conf key
                                 * no_pix_distrib, video_prediction/setup_predictor.py:110-114).  The weights do not depend
                                 * on ndesig.  See "Frames-only handles" below for what the entry points then expect. */
    int32_t n_context;          /* context frames (>= 1) */
    int32_t sequence_length;    /* n_context + T */
    int32_t num_masks;          /* CDNA kernel slots K (masks = K + 1): 10 for arch 0 / 1; 6 for arch 2 (four kernels in
                                 * the checkpoint, seven compositing layers); 4 for arch 3 (four kernels, seven layers); 1 for arch 0 with
                                 * layer_spec 3 (DNA: one transform, two mask channels) */
    int32_t max_batch;          /* run_batch_size: most samples per vf_rollout call */
    int32_t device;             /* HIP device ordinal */
    int32_t precision;          /* arithmetic of the conv-LSTM gate GEMMs (96 % of the work):
                                 * 0 = exact fp32 MFMA (default);
                                 * 1 = fp32 emulated with six bf16 MFMA products per multiply
                                 *     (3-way exact operand split, fp32 accumulate; fp32-class
                                 *     accuracy, see csrc/vf_conv_bf16x6.h);
                                 * 2 = plain bf16: activations and weights of the gate GEMMs rounded
                                 *     once (to nearest even) to bf16, ONE bf16 MFMA product per
                                 *     multiply, fp32 accumulate (half-precision accuracy class: the
                                 *     speed / accuracy trade of the reference's float16 predictor, see
                                 *     csrc/vf_conv_bf16.h).  1 and 2: arch 0 with layer_spec 0, arch 1.
                                 *     Everything else is fp32 in every mode. */
    int32_t ncam;               /* camera views (1..4; 0 = 1): one network (own weights) per view,
                                 * all rolled by the same launch on the same action sequences
                                 * (reference: IndepMultiSAVP..., vpred_model_interface.py:60-88) */
    int32_t n_draws;            /* latent draws per action (>= 1; 0 = 1): every n_draws consecutive
                                 * sequences of a rollout are draws of ONE action and their costs
                                 * are averaged on the device (the reference's hook repeats each
                                 * action stochastic_planning[0] times,
                                 * samplers/gaussian_sampler.py:140-141) */
    int32_t arch;               /* network: 0 = action-conditioned CDNA conv-LSTM (cdna_arch.py; height and
                                 * width multiples of 8); 1 = SAVP-class stochastic generator (savp_arch.py:
                                 * the same conv-LSTM core between one more encoder and decoder scale, the
                                 * first context frame as an extra compositing layer, the per-step latent as
                                 * extra action channels; multiples of 16); 2 = arch 1 moved closer to the
                                 * published SAVP generator (savp_arch.py, Savp2Config: the vector [action, latent,
                                 * state] conditions EVERY conv-LSTM - lstm weights [5][5][Cx + adim + sdim + Ch][4Ch] -
                                 * and the compositing is the published one: four CDNA kernels, layers [warps,
                                 * previous, first, scratch]; exact fp32 only, at least 64 x 64); 3 = the PUBLISHED SAVP
                                 * generator (savp3_arch.py; arXiv:1804.01523 appendix A: instance norm after every conv and
                                 * inside the conv-LSTM cells, conv + average pool / bilinear up-sampling + conv, the layer
                                 * table by image size, [action, state, rnn_z(latent)] tile-concatenated in front of every
                                 * conv and conv-LSTM, 3x3 heads, dependent masks, symmetric-padded CDNA warps; exact fp32
                                 * only).  The reference selects the class through conf['model'],
                                 * vpred_model_interface.py:52-58 */
    int32_t zdim;               /* arch 3: how many of the adim action channels are the per-step latent z_t (they go
                                 * through the rnn_z cell and do not reach the state predictor); 0 for arch 0 - 2 */
    int32_t layer_spec;         /* arch 3: 0 = encoder / decoder table by min(height, width) as the public code selects it;
                                 * 32 / 64 / 128 force a table (64 = the paper's five-cell network).  arch 0: 0 = the survey
                                 * table, 1 = the decoder widths of the public CDNA code, 2 = the survey table with
                                 * appearance-flow compositing (a 1x1 flow head and nine bilinearly gathered warps in place of
                                 * the CDNA FC and kernels; tensors flow/w, flow/b where cdna/w, cdna/b sit), 3 = the survey
                                 * table with DNA compositing (selector: arch 0, layer_spec 3, num_masks 1 - a 1x1 head predicts
                                 * a normalised 5x5 kernel per pixel; no rgb head, two mask channels, tensors dna/w [1][1][32][25],
                                 * dna/b where cdna/w, cdna/b sit), 4 = the survey
                                 * table with STP compositing (selector: arch 0, layer_spec 4, num_masks 10 - a two-layer FC head on
                                 * the bottleneck predicts nine affine transforms per sample, each a clamped bilinear warp of the
                                 * whole previous frame; tensors stp_fc/w [fc_in][100], stp_fc/b where cdna/w, cdna/b sit, then
                                 * stp/w [100][54], stp/b); 1 - 4 are exact fp32 only (precision 0).  0 for arch 1 - 2 */
} vf_config;

typedef struct vf_handle vf_handle;

int vf_abi_version(void);
const char *vf_last_error(void);

/* Frames-only handles (vf_config.ndesig == 0).  Every argument that carries or receives a designated-pixel quantity
 * must be NULL; a violation returns VF_ERR_INVALID with a vf_last_error() message that says "frames-only" and launches
 * nothing, and the handle stays usable:
 *   vf_set_context      d_ctx_distrib must be NULL
 *   vf_rollout          goal_pix, task_weights, d_scores, d_scores_per_task must be NULL; nothing is written for them
 *                       and no score reduction is launched
 *   vf_export           d_distrib must be NULL (frames and states as usual)
 *   vf_render_plans     d_distrib_u8 must be NULL (frames as usual; d_lut may be NULL)
 *   vf_ensemble_scores  refuses such members
 * vf_goal_image_scores, vf_scorer_scores, vf_debug_lstm_layer, vf_device_status, vf_register and the setters work
 * unchanged; an abandoned launch still turns the goal-image and scorer outputs into NaN.  Call sequence:
 *   vf_create(cfg with ndesig 0) - vf_load_weights - vf_set_context(h, frames, states, actions, NULL, st) -
 *   vf_rollout(h, d_actions, B, NULL, 0.f, NULL, NULL, NULL, st) - vf_goal_image_scores / vf_scorer_scores /
 *   vf_export(h, first, count, d_frames, NULL, d_states, st) / vf_render_plans(h, d_seq, K, NULL, d_frames_u8, NULL, st).
 * vf_create of such a config allocates no distribution tensor, no context-distribution buffer and no block-sum buffer. */

/* Number of float32 values of ONE view's weights for `cfg` (the canonical tensor table of
 * visual_foresight_amd/video_prediction/cdna_arch.py, concatenated in table order);
 * vf_load_weights expects ncam such blobs back to back. */
size_t vf_weight_count(const vf_config *cfg);

/* Build one engine: allocates every device buffer (weights, recurrent state, activations,
 * predictions for max_batch samples).  Replaces setup_predictor()'s graph/session build,
 * visual_mpc/video_prediction/setup_predictor.py:61-128. */
int vf_create(const vf_config *cfg, vf_handle **out);
int vf_destroy(vf_handle *h);

/* Upload network weights from a HOST blob in canonical layout (views back to back) and re-pack
 * them for the MFMA kernels into the buffers vf_create allocated; may be called again at any
 * time (hot swap; blocks until rollouts in flight have finished).  Replaces saver.restore /
 * model.restore, setup_predictor.py:130-145, and predictor.restore(),
 * pixel_cost_controller.py:34. */
int vf_load_weights(vf_handle *h, const float *host_blob, size_t n_floats);

/* Install the planning context (device pointers).  Replaces get_context(),
 * visual_mpc/video_prediction/pred_util.py:4-13 (last n_context frames, uint8 -> float/255) and
 * the batch-1 placeholders tiled per tower, setup_predictor.py:40-44: the context is kept once
 * and broadcast to every sample by the kernels, never materialised per sample.  A frames-only handle (ndesig 0) wants
 * d_ctx_distrib == NULL and refuses anything else. */
int vf_set_context(vf_handle *h, const uint8_t *d_frames, const float *d_states,
                   const float *d_ctx_actions, const float *d_ctx_distrib, void *stream);

/* Grouped contexts: G planning problems in one rollout.  Rows [g * rows_per_group, (g + 1) * rows_per_group) of every later vf_rollout read
 * context g.  Layouts: vf_set_context's with a leading [n_groups] axis.  d_ctx_distrib NULL on a frames-only handle.
 * Every context distribution plane is normalised, as vf_set_context expects.
 * The contexts are converted and expanded into one copy per row; a step reads them with a row stride where it reads the
 * broadcast context with stride 0, and the rollout is emitted as with vf_set_dedup(h, 0) whatever that switch says
 * (nothing is shared between rows; every route gives the bits G single-context rollouts of rows_per_group rows give).
 * While the handle is in this GROUPED MODE vf_rollout wants B == n_groups * rows_per_group and scores every row against
 * the one goal_pix it is passed (vf_group_pixel_scores takes a goal per group); vf_export, vf_render_plans,
 * vf_goal_image_scores, vf_scorer_scores and vf_device_status work on the rows unchanged.  A later vf_set_context
 * returns the handle to the broadcast mode.  The FIRST call on a handle allocates the per-row buffers (for max_batch
 * rows - the one exception to "no later call allocates"; vf_destroy frees them); every call enqueues one kernel on
 * `stream` and never synchronises.  Returns VF_ERR_INVALID (nothing launched, the handle as it was; the message names
 * "grouped contexts") for arch 1 .. 3, n_draws > 1, n_groups < 1, rows_per_group < 1, n_groups * rows_per_group >
 * max_batch, a d_ctx_distrib that contradicts ndesig, or missing context actions with n_context > 1. */
int vf_set_contexts(vf_handle *h, int32_t n_groups, int32_t rows_per_group, const uint8_t *d_frames,
                    const float *d_states, const float *d_ctx_actions, const float *d_ctx_distrib, void *stream);

/* Expected-distance cost of the handle's LAST vf_rollout against one goal per group, from the resident distributions.
 * d_goal_pix: DEVICE int32 [n_groups][ncam][ndesig][2] (row, col; may lie off-image).  task_weights: HOST float
 * [n_groups][ncam * ndesig] or NULL.  d_scores float64 [B], d_scores_per_task float64 [B][ncam * ndesig] (may be NULL).
 * Per row b of group g, view c, pixel p, step t:  S1 = sum over pixels of x * || (row, col) - goal[g][c][p] ||  over the
 * unnormalised distribution x (float64 root of the exact integer, float64 accumulation in an order that depends on H
 * and W alone: a row's cost has the same bits in any batch, group count or position), S0 the divisor vf_export
 * normalises with; then vf_rollout's reduction:  e = sum_t w_t (S1 / S0) / sum_t w_t,  w = (1, ..., 1, finalweight),
 * and the plain mean over tasks or the group's task_weights sum.  If the handle's device status is raised every output
 * is NaN.  Enqueues two kernels (with task_weights one more per 32 groups) on `stream`, allocates nothing, never
 * synchronises.  Returns VF_ERR_INVALID (nothing launched; the message names "grouped contexts") for a NULL handle /
 * d_goal_pix / d_scores, a frames-only handle, a handle outside grouped mode, or one that has not rolled since its
 * vf_set_contexts. */
int vf_group_pixel_scores(vf_handle *h, const int32_t *d_goal_pix, float finalweight, const float *task_weights,
                          double *d_scores, double *d_scores_per_task, void *stream);

/* Roll B (<= max_batch, a multiple of n_draws) action sequences through every view's predictor
 * for T steps and reduce the predicted designated-pixel distributions to costs on the device.
 * Replaces predictor_func()/sess.run, setup_predictor.py:164-200, the call at
 * pixel_cost_controller.py:83, and the host cost of pixel_cost_controller.py:135-197:
 *   e[b][c*ndesig+p] = sum_t w_t * E_{distrib[b,t,c,p]}[ || pix - goal_cp || ] / sum_t w_t,
 *   w = (1, ..., 1, finalweight);   score_b = mean over tasks of e[b][.]        (:153)
 * or, with task_weights (HOST float [ncam*ndesig], NULL = plain mean), the trade-off weighted
 * sum  score_b = sum_i task_weights[i] * e[b][i]  (register_gtruth_controller.py:88-94).  With
 * n_draws > 1 both are means over each action's draws.  goal_pix: HOST int32
 * [ncam][ndesig][2] (row, col).  d_scores_per_task may be NULL.  Predictions stay resident in
 * the handle until the next vf_rollout (see vf_export).  If a tile of the launch gave up
 * waiting for its producers (see vf_device_status) every score of this and of later rollouts
 * is NaN until the status has been read, and the predictions vf_export would copy out are
 * undefined (the launch was abandoned): check the scores or vf_device_status first.
 * Frames-only handles (ndesig 0): goal_pix, task_weights, d_scores and d_scores_per_task must all be NULL, nothing is
 * reduced or written for them; read vf_device_status, or the NaN of vf_goal_image_scores / vf_scorer_scores. */
int vf_rollout(vf_handle *h, const float *d_actions, int32_t B, const int32_t *goal_pix,
               float finalweight, const float *task_weights, double *d_scores,
               double *d_scores_per_task, void *stream);

/* Ensemble cost over independently trained predictors (reference
 * visual_mpc/policy/cem_controllers/variants/ensemble_vidpred.py:32-61).  Scores the LAST vf_rollout of every member -
 * n_members (1..16) handles of one vf_config, device included, that rolled the same sequences with the same goal pixels
 * (same B).  Per (view c, pixel p, rolled sequence, step t) member m's expected distance x_m is the value its own
 * vf_rollout scored with; the step cost is
 *   c_t = mean_m x_m + lambda_variance * var_m x_m          (population variance, two passes, members in list order)
 * and replaces x in vf_rollout's reduction: time-weighted mean with w = (1, ..., 1, finalweight), mean over the action's
 * n_draws sequences, plain mean over tasks or the task_weights sum.  d_scores [B / n_draws] and d_scores_per_task
 * [B / n_draws][ncam * ndesig] as vf_rollout's; d_cost_per_step (float64 [B / n_draws][ncam * ndesig][T], may be NULL)
 * receives c_t averaged over the draws.  d_scores_per_task may be NULL.  If any member's device status is raised every
 * output is NaN.  Enqueues one kernel on `stream` and never synchronises.
 * Drive every member from ONE stream, one rollout after the other, and score on that stream: two persistent rollouts
 * running at the same time can starve each other, their tiles give up waiting and every score becomes NaN.
 * Returns VF_ERR_INVALID (nothing launched) for a NULL / empty / too long member list, differing configs, a member
 * that has not rolled, differing B or differing goal pixels, or a frames-only member (ndesig 0: it keeps no sums). */
int vf_ensemble_scores(vf_handle *const *members, int32_t n_members, float lambda_variance, float finalweight,
                       const float *task_weights, double *d_scores, double *d_scores_per_task,
                       double *d_cost_per_step, void *stream);

/* Goal-image cost (reference visual_mpc/policy/cem_controllers/goal_im_controller.py:93: CEM on the mean squared error
 * between a predicted frame and a goal picture).  Scores the frames of the handle's LAST vf_rollout where they lie -
 * nothing is exported or copied.  d_goal: DEVICE float32 [ncam][H][W][3], 16-byte aligned, in the scale the host wants
 * compared with the predicted frames (which are in [0,1]).  Per rolled sequence b, view c, step t
 *   mse[b][c][t] = mean over (row, col, channel) of (frame[b][t][c] - goal[c])^2       (float64)
 * steps_mode 0: e[b][c] = mse[b][c][T-1], only the last predicted frames are read (unless d_cost_per_step asks for all);
 * steps_mode 1: e[b][c] = sum_t w_t mse[b][c][t] / sum_t w_t, w = (1, ..., 1, finalweight), the weighting of vf_rollout.
 * Then the mean over each action's n_draws sequences; score = e[.][0] if first_view_only, else the plain mean over views.
 * d_scores float64 [B / n_draws]; d_scores_per_view float64 [B / n_draws][ncam] (may be NULL); d_cost_per_step float64
 * [B / n_draws][ncam][T] = mse averaged over the draws (may be NULL).  The summation order of an image depends on H and W
 * alone: a sequence's cost has the same bits in any batch, chunk or rank.  If the handle's device status is raised every
 * output is NaN.  Enqueues two kernels on `stream` and never synchronises.  Returns VF_ERR_INVALID (nothing launched) for
 * a NULL handle / d_goal / d_scores, a misaligned d_goal, a steps_mode other than 0 or 1, or a handle that has not
 * rolled. */
int vf_goal_image_scores(vf_handle *h, const float *d_goal, int32_t steps_mode, float finalweight,
                         int32_t first_view_only, double *d_scores, double *d_scores_per_view,
                         double *d_cost_per_step, void *stream);

/* Plan visualisation (reference visual_mpc/policy/cem_controllers/pixel_cost_controller.py:88-131: the ten best plans of
 * a CEM iteration as movies).  Renders K rolled sequences of the handle's LAST vf_rollout where they lie, so that only
 * bytes leave the device.  d_seq: DEVICE int32 [K], indices into the rolled batch (an entry outside [0, B) is clamped
 * into it - the host validates before the upload).  d_lut: DEVICE uint8 [256][3], any colour table.  Outputs (either
 * may be NULL), one movie contiguous:
 *   d_frames_u8  [K][ncam][T][H][W][3]          = (uint8) trunc(frame * 255.0f)                          (:123)
 *   d_distrib_u8 [K][ncam][ndesig][T][H][W][3]  per plane, p the normalised distribution vf_export gives:
 *       mx = max over the plane of p;  q = p / (mx + 1e-6f)  (float32 add, IEEE float32 division);
 *       pixel = d_lut[min((int)(q * 256.0f), 255)]                                                       (:114-115)
 * Enqueues at most two kernels on `stream`, allocates nothing, never synchronises.  Returns VF_ERR_INVALID (nothing
 * launched) for a NULL handle / d_seq, both outputs NULL, d_distrib_u8 without d_lut, K < 1 or K > max_batch, a
 * handle that has not rolled, or d_distrib_u8 on a frames-only handle (ndesig 0). */
int vf_render_plans(vf_handle *h, const int32_t *d_seq, int32_t K, const uint8_t *d_lut, uint8_t *d_frames_u8,
                    uint8_t *d_distrib_u8, void *stream);

/* Learned-cost planning: a frame scorer on the device (reference
 * visual_mpc/policy/cem_controllers/variants/classifier_controller.py:34-36,94-105 and nce_cost_controller.py:33-35,90-103:
 * control_embedding.deploy_simple_model / deploy_model on a GPU of its own, every predicted frame copied to the host and
 * through that network).  The scorer package is not part of the reference snapshot; the network is this project's
 * (visual_foresight_amd/video_prediction/frame_scorer_arch.py: four 3x3 / 2 convolutions 32-64-128-128 with ReLU, mean
 * over the positions, FC to D values), one weight set per view.  head 0 = classifier (D = 2 logits; embed_dim ignored),
 * head 1 = embedding (D = embed_dim) with a second tower (tower 1, six input channels: concat[goal image, start image],
 * nce_cost_controller.py:94-99).  height and width are multiples of 16, width <= 128; max_frames = the most images
 * (per view) one call scores, e.g. the handle's max_batch * T.  Images are multiplied by input_scale (float32) on the way
 * in (classifier_controller.py:94,98: 1; nce_cost_controller.py:90,95: 255).  Every device buffer is allocated in
 * vf_scorer_create; vf_scorer_load_weights is the one blocking call.  The activations, head outputs and raw costs of a
 * pass are scratch of the scorer: like a handle, a scorer is driven from ONE stream at a time - two scoring or embedding calls
 * on the same scorer from different streams would overwrite each other's scratch (use one scorer per stream). */
typedef struct vf_scorer_config {
    int32_t height, width;
    int32_t ncam;               /* views (1..4; 0 = 1) */
    int32_t head;               /* 0 = classifier, 1 = embedding */
    int32_t embed_dim;          /* head 1: D (1..1024) */
    int32_t max_frames;
    int32_t device;             /* HIP device ordinal */
    float input_scale;
} vf_scorer_config;

typedef struct vf_scorer vf_scorer;

/* float32 values of ONE view's weights of `tower` (0: frames, 1: goal / start pair, head 1 only), the canonical table of
 * frame_scorer_arch.py concatenated in table order; 0 + vf_last_error() for a bad config or tower. */
size_t vf_scorer_weight_count(const vf_scorer_config *cfg, int32_t tower);
int vf_scorer_create(const vf_scorer_config *cfg, vf_scorer **out);
int vf_scorer_destroy(vf_scorer *s);
/* HOST blob, ncam views back to back; re-packs the convolution weights for the MFMA kernel into the buffers
 * vf_scorer_create allocated (replaces restore_path of deploy_simple_model / deploy_model). */
int vf_scorer_load_weights(vf_scorer *s, int32_t tower, const float *host_blob, size_t n_floats);
/* Any images: d_images DEVICE float32 [n][ncam][H][W][Cin] (Cin = 3 for tower 0, 6 for tower 1; 16-byte aligned; in the
 * scale of predicted frames, multiplied by input_scale like them) -> d_out [n][ncam][D].  n <= max_frames.  The goal /
 * start pair of nce_cost_controller.py:94-98 ('goal_enc'), and the tests. */
int vf_scorer_embed(vf_scorer *s, int32_t tower, const float *d_images, int32_t n, float *d_out, void *stream);
/* Scores the frames of h's LAST vf_rollout where they lie (nothing is exported or copied).  Per rolled sequence b and
 * step t:  raw[b][t] = sum over views c of x[b][t][c]                     (classifier_controller.py:104, nce_...:102)
 *   head 0: x = -log(p1 + 1e-5), p = softmax(logits) in float64 from the float32 logits                 (:10,102)
 *   head 1: x = -sum_d d_goal_enc[c][d] * enc[b][t][c][d], float64 products, d ascending        (nce_...:100,160-164)
 * then _weight_scores (classifier_controller.py:135-142): finalweight >= 0: (sum_{t<T-1} raw + fw * raw[T-1]) / (T-1+fw);
 * finalweight < 0: raw[T-1] (only the last frames are scored unless an optional output wants all); then the mean over
 * each action's n_draws sequences.  d_scores float64 [B / n_draws]; d_cost_per_step float64 [B / n_draws][T] = raw
 * averaged over the draws (NULL ok); d_head_out float32 [B][T][ncam][D] (NULL ok); d_goal_enc DEVICE float32 [ncam][D]
 * (head 1; ignored for head 0).  A frame's head output has the same bits in any batch, chunk or rank.  If the handle's
 * device status is raised every output is NaN.  Enqueues on `stream`, never synchronises, allocates nothing.
 * VF_ERR_INVALID (nothing launched): NULL s / h / d_scores, scorer and handle of different size / ncam / device, a handle
 * that has not rolled, more frames than max_frames, head 1 without d_goal_enc, weights not loaded. */
int vf_scorer_scores(vf_scorer *s, vf_handle *h, const float *d_goal_enc, float finalweight, double *d_scores,
                     double *d_cost_per_step, float *d_head_out, void *stream);

/* Registration network: the flow field of designated-pixel registration on the device (reference
 * visual_mpc/policy/cem_controllers/register_gtruth_controller.py:7,21,64-66: setup_gdn(gdnconf, gpu_id) builds the
 * warper, which is called once per registration target and planning call).  The registration_network package is not part
 * of the reference snapshot; the network is this project's
 * (visual_foresight_amd/video_prediction/registration_net_arch.py: 3x3 convolutions with ReLU, three with 2x2 max-pool
 * 6 -> 32m -> 64m -> 128m, three with bilinear x2 up-sampling -> 64m -> 32m -> 16m, a 5x5 flow head; m = ch_mult), one
 * weight set per view.  height and width are multiples of 8 in 16..128, ch_mult is 1, 2 or 4, max_pairs the most
 * (current, reference) pairs of one call.  Every device buffer is allocated in vf_regnet_create; vf_regnet_load_weights is
 * the one blocking call.  The activations are scratch of the net: like a scorer, a net is driven from ONE stream at a
 * time.  A pair's flow has the same bits whatever n, slot or call it is computed in. */
typedef struct vf_regnet_config {
    int32_t height, width;
    int32_t ncam;               /* views (1..4; 0 = 1) */
    int32_t ch_mult;            /* 1, 2 or 4 */
    int32_t max_pairs;
    int32_t device;             /* HIP device ordinal */
} vf_regnet_config;

typedef struct vf_regnet vf_regnet;

/* float32 values of ONE view's weights, the canonical table of registration_net_arch.py concatenated in table order;
 * 0 + vf_last_error() for a bad config. */
size_t vf_regnet_weight_count(const vf_regnet_config *cfg);
int vf_regnet_create(const vf_regnet_config *cfg, vf_regnet **out);
int vf_regnet_destroy(vf_regnet *r);
/* HOST blob, ncam views back to back; re-packs the convolution weights for the MFMA kernel into the buffers
 * vf_regnet_create allocated (replaces gdnconf['pretrained_model']). */
int vf_regnet_load_weights(vf_regnet *r, const float *host_blob, size_t n_floats);
/* d_current, d_reference: DEVICE float32 [n][ncam][H][W][3] in [0, 1], 16-byte aligned, n <= max_pairs; d_flow: DEVICE
 * float32 [n][ncam][H][W][2] = (dx, dy), 8-byte aligned.  d_flow + i * ncam * H * W * 2 is what vf_register takes for pair
 * i.  Enqueues on `stream`, never synchronises, allocates nothing.  VF_ERR_INVALID (nothing launched): a NULL pointer, a
 * misaligned pointer, n < 1 or n > max_pairs, weights not loaded. */
int vf_regnet_flow(vf_regnet *r, const float *d_current, const float *d_reference, int32_t n, float *d_flow,
                   void *stream);

/* Inverse-model policy: the action-inference network on the device (reference
 * visual_mpc/policy/inverse_models/inverse_model_base_controller.py:4,31-32: predictor_class(model_params_path, {}, n_gpus,
 * first_gpu) and restore(); :76-80: one call per replanning step with the start image, the goal image, the context actions
 * and the context frames of camera 0, which returns the next T actions).  The robonet.inverse_model package is not part of
 * the reference snapshot; the network is this project's (visual_foresight_amd/video_prediction/inverse_model_arch.py: two
 * towers of the frame scorer's four 3x3 / 2 convolutions with a mean over the positions - `pair` on concat[goal, start],
 * `ctx` on every context frame - and an LSTM cell of 128 units, warmed up on the context, that decodes n_actions actions).
 * height and width are multiples of 16, width at most 128, adim 1..8, n_context 1..4, n_actions 1..32, max_batch the most
 * problems of one call.  Every device buffer is allocated in vf_invmodel_create; vf_invmodel_load_weights is the one
 * blocking call.  The activations are scratch of the model: like a scorer, a model is driven from ONE stream at a time.  A
 * problem's actions have the same bits whatever n, slot or call they are computed in. */
typedef struct vf_invmodel_config {
    int32_t height, width, adim, n_context, n_actions, max_batch, device;
    float input_scale;          /* the images are multiplied by this (float32) before c1 */
} vf_invmodel_config;

typedef struct vf_invmodel vf_invmodel;

/* float32 values of the weights, the canonical table of inverse_model_arch.py concatenated in table order; 0 +
 * vf_last_error() for a bad config. */
size_t vf_invmodel_weight_count(const vf_invmodel_config *cfg);
int vf_invmodel_create(const vf_invmodel_config *cfg, vf_invmodel **out);
int vf_invmodel_destroy(vf_invmodel *m);
/* HOST blob; re-packs the convolution weights for the MFMA kernel into the buffers vf_invmodel_create allocated (replaces
 * the restore() of the reference's predictor). */
int vf_invmodel_load_weights(vf_invmodel *m, const float *host_blob, size_t n_floats);
/* All DEVICE float32.  d_start, d_goal [n][H][W][3] and d_ctx_frames [n][n_context][H][W][3] in [0, 1], 16-byte aligned;
 * d_ctx_actions [n][n_context][adim]; d_actions [n][n_actions][adim]; d_hidden (may be NULL)
 * [n][n_context + n_actions][2][128] = h and c after every step of the recurrence (tests localise an error with it).
 * Enqueues a fixed number of launches on `stream` whatever n_actions is, never synchronises, allocates nothing.
 * VF_ERR_INVALID (nothing launched): a NULL pointer, a misaligned image pointer, n < 1 or n > max_batch, weights not
 * loaded. */
int vf_invmodel_infer(vf_invmodel *m, const float *d_start, const float *d_goal, const float *d_ctx_frames,
                      const float *d_ctx_actions, int32_t n, float *d_actions, float *d_hidden, void *stream);

/* Copy the predictions of the last vf_rollout out in the reference's layout (camera axis,
 * normalised distributions).  Any destination may be NULL.  first/count select a range of rolled
 * sequences.  Replaces the gen_images/gen_distrib/gen_states fetch of
 * setup_predictor.py:155-200.  A frames-only handle (ndesig 0) wants d_distrib == NULL and refuses anything else. */
int vf_export(vf_handle *h, int32_t first, int32_t count, float *d_frames, float *d_distrib,
              float *d_states, void *stream);

/* Designated-pixel registration (reference
 * visual_mpc/policy/cem_controllers/register_gtruth_controller.py:54-173, get_warp_err).  The
 * registration network is vf_regnet above (or any other source of a flow field); this entry point
 * takes its output, a flow field d_flow [ncam][H][W][2] = (dx, dy) that maps reference pixel (r, c) to the point
 * (x, y) = (c + dx, r + dy) of the current frame, and does the rest on the device:
 *   d_warp_pts [ncam][H][W][2] = (x, y)                        (optional, may be NULL)
 *   d_warped   [ncam][H][W][3] = bilinear sample of d_current at warp_pts, border-clamped (opt.)
 *   per (camera, task) with designated/goal pixel d_pix [ncam][ntask][2] (row, col, int32,
 *   DEVICE) in the reference image:
 *     region == 0: d_desig = flipped warp_pts at the pixel (:129-135), d_err = L2 photometric
 *                  error between d_reference and the warped frame at the pixel (:163-170);
 *     region  > 0: d_desig = per-coordinate MEDIAN of warp_pts over the (2*region+1)^2 window,
 *                  d_err = mean squared error over the window (:139-161); the window is clipped
 *                  to [0, size - clip_sub] (the reference clips the start window with 1, the goal
 *                  window with 0).
 * d_desig float [ncam][ntask][2] (row, col), d_err float [ncam][ntask].  ncam/H/W are the
 * handle's.  The trade-off weights (1/err normalised over cameras and registrations, :88-91)
 * are a handful of numbers and stay on the host. */
int vf_register(vf_handle *h, const float *d_current, const float *d_reference, const float *d_flow,
                const int32_t *d_pix, int32_t ntask, int32_t region, int32_t clip_sub,
                float *d_warped, float *d_warp_pts, float *d_desig, float *d_err, void *stream);

/* vf_register at a size of the caller's.  The reference registers at the AGENT's resolution and predicts at the
 * network's: the medium-resolution pixel tables of register_gtruth_controller.py:183,191, get_warp_err :121-128 on the
 * agent-size frames, the window clipped with the agent's dimensions (:144-155), the tracked pixels scaled back by
 * img_height / image_height (:172).  Same kernels and arguments as vf_register, the handle's ncam and device, but every
 * image and the flow are [ncam][H][W][.] with the caller's H, W (each at least 8, H * W <= 2^22), the pixels d_pix and
 * the results d_desig are in those coordinates and the window is clipped to [0, H - clip_sub] x [0, W - clip_sub].
 * Called with the handle's own size it gives vf_register's bits.  VF_ERR_INVALID (nothing launched): vf_register's
 * refusals, H < 8 or W < 8. */
int vf_register_hw(vf_handle *h, int32_t H, int32_t W, const float *d_current, const float *d_reference,
                   const float *d_flow, const int32_t *d_pix, int32_t ntask, int32_t region, int32_t clip_sub,
                   float *d_warped, float *d_warp_pts, float *d_desig, float *d_err, void *stream);

/* Area resampling: shrink n NHWC images [n][Hs][Ws][C] to [n][Hd][Wd][C] on the device (reference
 * visual_mpc/utils/im_utils.py:6-15 and agent/general_agent.py:128: every observation goes through
 * cv2.resize(..., INTER_AREA) before the policy sees it; goal_im_controller.py:89 the goal picture;
 * register_gtruth_controller.py:44-51 the context of the two-resolution registration controller).  Handle-free: `device`
 * is the HIP ordinal; one kernel is enqueued on `stream`, nothing is allocated, nothing synchronises.  dtype 0 = uint8,
 * 1 = float32 (source and destination alike); C in 1..4; Hd <= Hs and Wd <= Ws, any ratio; equal sizes give a copy (below).
 * The result is the EXACT area average (csrc/vf_resize.h; this project's own specification - it is meant to be
 * INTER_AREA for shrinking, but cv2 was not available to pin that, and OpenCV's integer-factor fast path may round ties
 * differently).  Per axis the weights are integers: destination row i covers [i*Hs, (i+1)*Hs), source row r covers
 * [r*Hd, (r+1)*Hd), wy[i][r] = the length of the overlap (sum_r wy = Hs), wx likewise (sum_c wx = Ws), A = Hs*Ws.
 *   uint8:   S = sum_r sum_c wy*wx*v (an exact integer);  out = S / A rounded half to even.
 *   float32: one float64 sum per output element, source rows ascending and columns ascending within a row, every term
 *            (double)(wy*wx) * (double)v (exact), additions rounded to nearest and never contracted; then one float64
 *            division by A and one rounding to float32.
 * An image's output depends on that image and the two sizes alone - not on n, its slot, the stream or the alignment.
 * VF_ERR_INVALID (nothing launched, the device is not touched): a NULL pointer, dtype not 0 / 1, n < 1, C outside 1..4,
 * a destination larger than the source on either axis, Hs*Ws > 2^22 (the uint8 sum must fit 31 bits), float32 pointers
 * that are not 4-byte aligned, n * Hd > 2^30 (the grid of the one launch).  Equal sizes: uint8 is copied exactly; float32
 * keeps every value but not every bit (-0.0 comes back as +0.0: the sum starts at +0.0). */
int vf_resize_area(int32_t device, const void *d_src, void *d_dst, int32_t dtype /*0 = uint8, 1 = float32*/,
                   int32_t n, int32_t Hs, int32_t Ws, int32_t C, int32_t Hd, int32_t Wd, void *stream);

/* Device-resident CEM iteration (csrc/vf_cem.h): pick the elites of a rollout's scores, refit the Gaussian proposal on them
 * and draw the next candidates - all on the caller's stream, so that the iterations of one planning call (reference
 * visual_mpc/policy/cem_controllers/cem_base_controller.py:85-116, samplers/gaussian_sampler.py:75-150, both host NumPy)
 * need no download between rollouts.  The arithmetic is specified by the float64 class
 * visual_foresight_amd/policy/cem_controllers/samplers/philox_gaussian_sampler.py: Philox4x32-10 under the key
 * {seed_lo, seed_hi} with the counter {block j, trial n, sample i, call}; Box-Muller in float64; the proposal in factor
 * form sigma = A A^T with the draw x_d = mean_d + sum_r A[d][r] z_r as one fma chain, r ascending.
 * Handle-free like vf_resize_area: `device` is the HIP ordinal, nothing is allocated, nothing synchronises.
 * D = nactions * adim <= 128, T = nactions * repeat, a row of d_actions holds adim + tail <= 8 floats, 2 <= n_elites <= 256.
 * Workspace (caller-owned, vf_cem_workspace_bytes, 16-byte aligned): int32 R, int32 pad[3]; double mean[D];
 * double A[max(D, n_elites)][D] with A[d][r] at [r][d].  The FIRST proposal of a planning call is uploaded by the caller
 * in that layout (R = D, A = diag(std): any async copy on the same stream); vf_cem_refit writes the later ones. */
typedef struct vf_cem_config {
    int32_t nactions, repeat, adim, tail;
    int32_t n_elites;
    int32_t max_trials;         /* >= 1: draws per sample before the last one is clipped into rej_lim */
    int32_t rejection;          /* 0: the first draw is taken as it is */
    int32_t zero_first;         /* sample 0 becomes the zero action (its appended constants stay) */
    int32_t discrete_mask;      /* bit c: column c becomes clip(floor(x), 0, 4) */
    uint32_t seed_lo, seed_hi;
    int32_t reserved;
    double rej_lim[8];          /* per action column: |x| <= rej_lim accepts; +inf = no limit */
    double trunc_lim[8];        /* per action column: clip to +-trunc_lim after discretisation; +inf = none */
    double tail_value[8];       /* the constants written to columns adim .. adim + tail - 1 */
} vf_cem_config;

/* Bytes of the workspace for cfg; 0 (and vf_last_error) for an invalid cfg. */
size_t vf_cem_workspace_bytes(const vf_cem_config *cfg);

/* Elites and refit.  d_scores [M] float64 (as vf_rollout writes them), d_actions [M][T][adim + tail] float32 (the rollout's
 * input), n_elites <= M <= 4096.  Writes d_elite_index [n_elites] (the n_elites smallest scores in ascending (score, index)
 * order, NaN last), d_elite_score [n_elites], d_elite_plans [n_elites][T][adim + tail] (copies of the elites' rows) and,
 * into the workspace, R = n_elites, mean_d = (sum over the elites in rank order of their value at the LAST step of held
 * action d) / n_elites and A[d][k] = (e_kd - mean_d) / sqrt(n_elites - 1), float64, each operation rounded once.
 * One kernel of one workgroup.  VF_ERR_INVALID (nothing launched): a NULL pointer, an invalid cfg, M outside the range. */
int vf_cem_refit(int32_t device, const vf_cem_config *cfg, const double *d_scores, const float *d_actions, int32_t M,
                 int32_t *d_elite_index, double *d_elite_score, float *d_elite_plans, void *d_workspace, void *stream);

/* Draw M <= 4096 candidates from the workspace's proposal as sampling call number `call` (word 3 of the counter).  Writes
 * d_actions [M][T][adim + tail] float32 - every sampled action held for `repeat` steps, the constants in the tail columns -
 * d_trials [M] (draws taken) and d_capped [M] (1: max_trials draws were rejected and the last one was clipped).  One
 * wavefront per sample; the only data-dependent loop is the trial loop, bounded by max_trials.
 * VF_ERR_INVALID (nothing launched): a NULL pointer, an invalid cfg, M outside 1..4096. */
int vf_cem_sample(int32_t device, const vf_cem_config *cfg, const void *d_workspace, uint32_t call, int32_t M,
                  float *d_actions, int32_t *d_trials, int32_t *d_capped, void *stream);

/* The same for the time-correlated noise proposal of the RoboNet-era experiments (reference
 * visual_mpc/policy/cem_controllers/samplers/correlated_noise.py:10-80): i.i.d. normals through an AR(1) filter along the
 * action steps, refitted by an exponentially weighted soft mean of the elites.  The arithmetic is specified by the float64
 * class visual_foresight_amd/policy/cem_controllers/samplers/philox_correlated_sampler.py: the white normal of sample i at
 * d = a * adim + c is normal d of the counter {block d / 4, 0, sample i, call}; shaped s_d = w_d * std[c] + bias[c], or with
 * refit_cov after a refit y_k = sum_d w_d A[d][k], s_d = sum_k A[d][k] y_k (two fma chains from 0, d then k ascending);
 * filtered o_a = (beta_0 * s_a) + (beta_1 * prev), prev = o_{a-1}, for a = 0 the unfiltered s_{nactions-1} or, with
 * has_first_prev, first_prev[c]; a candidate is o, plus centre once the workspace holds one.  No repeat: T = nactions.
 * D = nactions * adim <= 128, adim + tail <= 8, 1 <= n_elites <= 256 (2 with refit_cov).
 * Workspace (caller-owned, vf_cem_corr_workspace_bytes, 16-byte aligned): int32 R, int32 centre_valid, int32 pad[2];
 * double centre[D]; double mean[D]; double soft[n_elites]; with refit_cov double A[n_elites][D], A[d][k] at [k][d].
 * The caller starts a planning call by zeroing the 16-byte header (any async copy on the same stream): centre invalid, R 0. */
typedef struct vf_cem_corr_config {
    int32_t nactions, adim, tail, n_elites;
    int32_t refit_cov;          /* the refit also fits A, which then colours the noise in place of std and bias */
    int32_t has_first_prev;     /* step 0 is smoothed against first_prev, not against the last noise step */
    uint32_t seed_lo, seed_hi;
    double kappa, beta_0, beta_1;
    double std[8], bias[8];     /* per action column */
    double first_prev[8];
    double tail_value[8];       /* the constants written to columns adim .. adim + tail - 1 */
} vf_cem_corr_config;

/* Bytes of the workspace for cfg; 0 (and vf_last_error) for an invalid cfg. */
size_t vf_cem_corr_workspace_bytes(const vf_cem_corr_config *cfg);

/* Elites and soft refit.  Arguments and elite outputs as vf_cem_refit, with T = nactions.  Into the workspace:
 * soft_k = exp(kappa * (score_0 - score_k)) in rank order, centre_d = (sum_k e_kd * soft_k) / (sum_k soft_k + 1e-4),
 * centre_valid = 1 and, with refit_cov, R = n_elites, the plain mean and A as vf_cem_refit fits them (else R = 0).
 * One kernel of one workgroup.  VF_ERR_INVALID (nothing launched): a NULL pointer, an invalid cfg, M outside the range. */
int vf_cem_soft_refit(int32_t device, const vf_cem_corr_config *cfg, const double *d_scores, const float *d_actions,
                      int32_t M, int32_t *d_elite_index, double *d_elite_score, float *d_elite_plans, void *d_workspace,
                      void *stream);

/* Draw M <= 4096 candidates as sampling call number `call`: d_actions [M][nactions][adim + tail] float32.  One wavefront per
 * sample, no data-dependent loop.  VF_ERR_INVALID (nothing launched): a NULL pointer, an invalid cfg, M outside 1..4096. */
int vf_cem_sample_corr(int32_t device, const vf_cem_corr_config *cfg, const void *d_workspace, uint32_t call, int32_t M,
                       float *d_actions, void *stream);

/* The folding proposal of the towel experiments (reference visual_mpc/policy/cem_controllers/samplers/folding_sampler.py:7-132):
 * besides plain Gaussian draws, two scripted families of "lift, carry to a place, put down" plans.  The arithmetic is
 * specified by the float64 class visual_foresight_amd/policy/cem_controllers/samplers/philox_folding_sampler.py.  adim is 4.
 * The proposal, its workspace and its refit are vf_cem_config's: size the workspace with vf_cem_workspace_bytes and refit with
 * vf_cem_refit under a vf_cem_config of adim = 4 and the same nactions, repeat, tail and n_elites; upload the first proposal
 * as for vf_cem_sample.  Sample i < n_scripted is TWO_PLACES (carry + up, down, up, carry + up, down; later steps zero),
 * i < 2 n_scripted ONE_PLACE (up, carry + up, down, rest held to the end), the rest the plain draw of vf_cem_sample's trial
 * 0.  Counter {block, trial, sample i, call}: trial 1, block 0 gives the places u_j = word_j / 2^32 (first (u_0, u_1), second
 * (u_2, u_3)); trial 2 + s the R normals of scripted step s, v_c = m_c + g_c * sum_r A[c][r] z_r (an fma chain from 0 over
 * rows 0..3 of A), g = 1 on a carry and (sqrt(.1), sqrt(.1), 1, sqrt(.5)) on the spot, m = (dx, dy, lift, 0) with the carry
 * (end - start) / repeat.  Columns 0..2 are clipped to +-max_shift. */
typedef struct vf_cem_fold_config {
    int32_t nactions, repeat, tail;     /* 5 <= nactions <= 32; a row of d_actions holds 4 + tail <= 8 floats */
    int32_t n_elites;
    int32_t n_scripted;                 /* samples of each scripted family: 1 <= 2 * n_scripted <= M */
    int32_t reserved;
    uint32_t seed_lo, seed_hi;
    double start_xy[2];                 /* the gripper's xy at the start of the planning call: where the carries start */
    double max_shift[3];                /* clip of x, y, z; +inf = none */
    double tail_value[8];               /* the constants written to columns 4 .. 4 + tail - 1 */
} vf_cem_fold_config;

/* Draw M <= 4096 candidates as sampling call number `call`: d_actions [M][nactions * repeat][4 + tail] float32.  One
 * wavefront per sample, no data-dependent loop.  VF_ERR_INVALID (nothing launched): a NULL pointer, an invalid cfg, M outside
 * 2 * n_scripted..4096. */
int vf_cem_sample_fold(int32_t device, const vf_cem_fold_config *cfg, const void *d_workspace, uint32_t call, int32_t M,
                       float *d_actions, void *stream);

/* The autograsp proposal (reference visual_mpc/policy/cem_controllers/samplers/autograsp_sampler.py:5-58): a Gaussian proposal
 * over the moves whose last action column, the gripper command, is not sampled but derived from the planned height.  The
 * arithmetic is specified by the float64 class visual_foresight_amd/policy/cem_controllers/samplers/philox_autograsp_sampler.py.
 * The proposal, its workspace and its refit are vf_cem_config's: cfg->adim counts the MOVES (at least 3: column 2 is the
 * lift), cfg->tail >= 1 counts the gripper column (column adim; tail_value[0] is not read) and the appended constants behind
 * it (tail_value[1 ..]); size the workspace with vf_cem_workspace_bytes, refit with vf_cem_refit and upload the first
 * proposal as for vf_cem_sample, all under that cfg.  The moves are vf_cem_sample's of the same cfg, counter and workspace.
 * Height mode, per sample, from the float32 moves z_t that are stored: c_0 = float64(z_0) * action_norm_factor,
 * c_t = c_(t-1) + float64(z_t) * action_norm_factor, shut_t = c_t + state_z < z_thresh, every operation rounded once; unless
 * reopen the gripper stays shut from the first shut step on; then, with deviation_prob > 0, step t is flipped when
 * u_t < deviation_prob, u_t = word (t % 4) / 2^32 of the counter {block t / 4, 0xFFFFFFFE, sample i, call} - a trial word no
 * sampler and no latent draw uses.  Share mode (a refit that keeps the elites' gripper): share_t = float32(elites whose
 * gripper value at step t is float32(close_cmd)) / float32(n_elites), shut_t = u_t < share_t; no latch, no deviation.
 * The column holds float32(close_cmd) where shut, float32(open_cmd) elsewhere. */
typedef struct vf_cem_grip_config {
    int32_t mode;               /* 0: by height, 1: by the elites' share */
    int32_t reopen;             /* height mode: the gripper may open again once it has shut */
    double state_z;             /* the height the planning call starts from */
    double action_norm_factor;  /* lift action -> height */
    double z_thresh;            /* shut below this height */
    double deviation_prob;      /* height mode: chance of flipping a step, in [0, 1] */
    double close_cmd, open_cmd;
} vf_cem_grip_config;

/* Draw M <= 4096 candidates as sampling call number `call`: d_actions [M][nactions * repeat][adim + tail] float32 - moves,
 * gripper, appended constants - d_trials [M] and d_capped [M] as vf_cem_sample.  Share mode first computes d_share [T]
 * (float32, caller-owned scratch) from d_elite_plans [n_elites][T][adim + tail] (as vf_cem_refit wrote them) in a kernel of
 * one workgroup on the same stream; height mode reads neither and both may be NULL.  One wavefront per sample; the only
 * data-dependent loop is the trial loop, bounded by max_trials.
 * VF_ERR_INVALID (nothing launched): a NULL cfg, grip or pointer, a workspace that is not 16-byte or another pointer that is
 * not 4-byte aligned, an invalid cfg, adim < 3, tail < 1, M outside 1..4096, a mode other than 0 / 1, deviation_prob outside
 * [0, 1] or NaN, share mode without d_elite_plans or d_share. */
int vf_cem_sample_autograsp(int32_t device, const vf_cem_config *cfg, const vf_cem_grip_config *grip, const void *d_workspace,
                            uint32_t call, int32_t M, const float *d_elite_plans, float *d_share, float *d_actions,
                            int32_t *d_trials, int32_t *d_capped, void *stream);

/* The latent draws of a stochastic predictor on the device (BASELINE config 5: every candidate is rolled n_latent times with
 * common random numbers).  The arithmetic is specified by philox_latents / fold_latents of
 * visual_foresight_amd/video_prediction/stochastic_predictor.py.  vf_cem_latents writes d_z [n_latent][T][zdim] float32:
 * z[d][t][j] is normal t * zdim + j of the counter {block, 0xFFFFFFFF, d, call} under the key {seed_lo, seed_hi} - Philox
 * and Box-Muller as in vf_cem_sample, with a trial word no sampler uses, so the latents share no counter with the candidates
 * when the seeds and call numbers are equal.  One wavefront per draw, no data-dependent loop.
 * VF_ERR_INVALID (nothing launched): a NULL or not 4-byte aligned pointer, a negative device, n_latent, T or zdim < 1,
 * T * zdim > 2^30. */
int vf_cem_latents(int32_t device, uint32_t seed_lo, uint32_t seed_hi, uint32_t call, int32_t n_latent, int32_t T,
                   int32_t zdim, float *d_z, void *stream);

/* Fold the draws into the sample axis, draw-minor: d_seqs [M * n_latent][T][width + zdim] float32, row a * n_latent + d =
 * [d_actions[a] | d_z[d]] per step, from d_actions [M][T][width] (as vf_cem_sample* write them, width = adim + tail) and d_z
 * [n_latent][T][zdim].  Pure copying; 16-byte accesses when width and zdim are multiples of four and the three pointers are
 * 16-byte aligned.  VF_ERR_INVALID (nothing launched): a NULL or not 4-byte aligned pointer, a negative device, M, n_latent,
 * T, width or zdim < 1, M * n_latent rows or T * (width + zdim) floats per row that do not fit in int32. */
int vf_cem_fold_latents(int32_t device, const float *d_actions, const float *d_z, int32_t M, int32_t n_latent, int32_t T,
                        int32_t width, int32_t zdim, float *d_seqs, void *stream);

/* The one collective of multi-GPU planning: all-gather every rank's n_local score values (float64)
 * (n_local equal on all ranks: pad ragged shards) into d_all [world * n_local] with RCCL over
 * xGMI, on the caller's stream.  nccl_comm is the caller's ncclComm_t (one rank per GPU).  The
 * reference instead concatenates whole predicted videos of its towers on the host,
 * visual_mpc/video_prediction/setup_predictor.py:155-162.  RCCL is bound with dlopen at first use,
 * so the library has no link-time dependency on it. */
int vf_allgather_scores(vf_handle *h, void *nccl_comm, const double *d_local, int32_t n_local,
                        double *d_all, void *stream);

/* One host thread driving several GPUs (the reference's in-process towers: `ngpu` GPUs behind one
 * policy object, visual_mpc/video_prediction/setup_predictor.py:70,117-123).  vf_comm_init_all
 * creates one RCCL communicator per listed device (ncclCommInitAll; devices distinct) with the same
 * library instance vf_allgather_scores uses; vf_allgather_scores_group issues the all-gather of
 * every local rank - handle hs[i] on device hs[i]'s, communicator comms[i], stream streams[i]
 * (streams NULL = default streams) - inside one ncclGroupStart / ncclGroupEnd, which is how a single
 * thread must drive several ranks.  vf_comm_destroy releases one communicator. */
int vf_comm_init_all(int32_t n, const int32_t *devices, void **comms);
int vf_comm_destroy(void *comm);
int vf_allgather_scores_group(int32_t n, vf_handle *const *hs, void *const *comms,
                              const double *const *d_local, int32_t n_local, double *const *d_all,
                              void *const *streams);

/* Persistent rollout (no reference counterpart).  When enabled vf_rollout runs ALL steps, layers
 * and samples as one persistent launch whose workgroups draw tiles from a ticket queue and
 * honour per-sample dependencies, so the tail of one layer overlaps the head of the next
 * (visual_foresight_amd/csrc/vf_persistent.h).  Results are bit-identical to the per-layer
 * launches.  A tile that waits too long for its producers (a bounded spin, ~seconds) raises a
 * STICKY device status word: from then on every score is NaN.  vf_device_status synchronises
 * the device, returns the word (0 = healthy) and, if it was raised, re-arms it and drops the
 * cached context-only part of the network (the abandoned launch may have left it half-written),
 * so a retry recomputes it. */
int vf_set_persistent(vf_handle *h, int32_t enable);
int vf_device_status(vf_handle *h, int32_t *status);

/* XCD-aware ticket queues of the persistent rollout (default on; no reference counterpart).  The items
 * of every phase are dealt to one queue per XCD so that an output-channel group's weight slice and a
 * sample's neighbouring tiles are served from ONE XCD's L2; a workgroup draws from the queue of the XCD
 * it runs on and steals from the others once its own is empty.  Placement only affects speed: results
 * are bit-identical with one queue (enable = 0), which is the plain phase order. */
int vf_set_xcd_queues(vf_handle *h, int32_t enable);

/* Fused items of the persistent rollout (default on; no reference counterpart).  (1) The last transposed convolution and the
 * compositing of the next frame become ONE item per tile: the tile stays in registers / LDS, its LayerNorm partial
 * is published, the item waits for the sample's other tiles and composes its pixels itself - the full-resolution
 * decoder tensor is never written to memory (visual_foresight_amd/csrc/vf_fused_top.h).  Same arithmetic on the same
 * values: results are bit-identical to the two-phase schedule and to the per-layer launches.  (2) The two convolutions of
 * the 8 x 8 bottleneck (3x3 / 2, then 1x1 with the tiled action / state entering as a per-sample bias) become one item per
 * row tile: the first conv's tile holds whole images and all 64 channels, goes through LDS instead of memory and feeds the
 * second GEMM in its stand-alone K order (conv_pair_epilogue, visual_foresight_amd/csrc/vf_conv_mfma.h) - one dependency
 * hop per sample-step less, bit-identical as well.  enable = 0 switches both off (A/B measurements, tests). */
int vf_set_fuse_top(vf_handle *h, int32_t enable);

/* Scheduling options of the persistent rollout that change timing only, never results (no reference counterpart; round 5).
 *   VF_OPT_YIELD_BUDGET (0): cooperative CU-level priority - the recurrent half of an early-started conv-LSTM item sleeps
 *       while the other workgroup of its CU runs chain-critical work, at most `value` polls of ~0.4 us per item
 *       (visual_foresight_amd/csrc/vf_conv_mfma.h, "yielding"); 0 = off, -1 = automatic (on for small shards).
 *   VF_OPT_WRITE_THROUGH (1): tiles with 16-byte epilogue stores publish their outputs as sc1 (write-through) stores and
 *       skip the release fence in front of their completion counters; 0 = plain stores + release, 1 = on (default).
 * Exists for A/B measurements and for the tests that hold every setting to the same bits. */
#define VF_OPT_YIELD_BUDGET 0
#define VF_OPT_WRITE_THROUGH 1
int vf_set_sched_option(vf_handle *h, int32_t option, int32_t value);

/* Context de-duplication (default on).  While a step's inputs are context, part of the network
 * sees identical inputs for every sample (step < n_context-1: everything; step < n_context: the
 * encoder up to enc2); those launches then run once with batch 1 and are broadcast.  The
 * per-sample arithmetic is unchanged, results are bit-identical either way; the switch exists
 * for A/B measurements. */
int vf_set_dedup(vf_handle *h, int32_t enable);

/* Measurement hooks (no reference counterpart).  While enabled, every launch of the dominant
 * kernel - the persistent rollout, or the fused conv-LSTM gate GEMM of the per-layer path - is
 * bracketed by HIP events on its launch stream (host-side event objects are created on demand).
 * vf_get_profile waits for them and returns: kernel_ms = sum of the per-launch durations,
 * busy_ms = time during which at least one such launch was in flight (== kernel_ms when
 * launches do not overlap), the number of launches and their algorithmic FLOPs
 * (2 * B*H*W * 25*(Cx+Ch) * 4C each); then it resets the counters. */
int vf_set_profiling(vf_handle *h, int32_t enable);
int vf_get_profile(vf_handle *h, double *kernel_ms, int64_t *launches, double *flops,
                   double *busy_ms);

/* Introspection for tests/benchmarks: algorithmic multiply-accumulates of one sample-step. */
double vf_macs_per_sample_step(const vf_config *cfg);

/* Debug hooks: per-phase wait/run ticks of the persistent launch (tools/persist_stats.py), and a
 * switch that raises the device status word by hand (tests of the in-band failure path). */
int vf_set_phase_stats(vf_handle *h, int32_t enable);
int vf_debug_phase_stats(vf_handle *h, int32_t max_phases, int32_t *types, int32_t *items,
                         uint64_t *wait_run);
int vf_debug_poison_status(vf_handle *h);
/* Debugging aid: conv-LSTM `layer` (0..6 = lstm1..lstm7; arch 0 / 1) as ONE per-layer launch on caller-owned NHWC
 * device tensors, with the loaded weights of view 0 and the tile of the handle's own precision: d_x [B][h][w][Cx] is
 * taken as it is (no producer LayerNorm, no relu), d_h / d_c [B][h][w][C] are the previous hidden and cell state,
 * d_h_out / d_c_out receive the new ones.  B <= max_batch.  Uses the handle's statistics buffers: the rollout state
 * is UNDEFINED afterwards until the next vf_set_context.  Allocates nothing and never synchronises. */
int vf_debug_lstm_layer(vf_handle *h, int32_t layer /*0..6 = lstm1..lstm7*/, int32_t B,
                        const float *d_x, const float *d_h, const float *d_c,
                        float *d_h_out, float *d_c_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_H */
