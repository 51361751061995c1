/*
 * promp_hip.h -- C ABI of libpromp_hip.so, the MI355X (gfx950) implementation of the ProMP
 * meta-RL training hot path:
 *
 *     MetaSampleProcessor.process_samples -> MAMLAlgo._adapt -> ProMP.optimize_policy
 *
 * The reference (jonasrothfuss/ProMP) is pure Python/TF1 and has no FFI; this header is the
 * boundary a maintainer would bind with ctypes from the reference's plugin classes (see
 * INTEGRATION.md).  Each entry point cites the reference code it replaces, paths relative to
 * meta_policy_search/ in the reference tree.
 *
 * Conventions
 *   - return 0 on success, negative on failure; promp_last_error() has the message
 *     (thread-local, valid until the next call on the thread).
 *   - the caller owns every host buffer (C-contiguous); the library owns device memory in ctx.
 *   - float32 unless noted; parameters cross the boundary as ONE flat vector [Theta] in the
 *     reference's OrderedDict order (policies/base.py:271-277): hidden_0/kernel [O,H1] row-major
 *     (x @ W convention, policies/networks/mlp.py:101), hidden_0/bias, hidden_1/kernel,
 *     hidden_1/bias, output/kernel [H2,A], output/bias, log_std_var [A].
 *   - work is enqueued on the context's HIP stream; calls that hand data back to the host
 *     synchronise before returning, the others return once the work is enqueued.
 *   - one ctx per GPU per process; not thread-safe (the reference's host is single-threaded).
 *   - there is NO CPU fallback: with no usable HIP device promp_ctx_create fails.
 */
#ifndef PROMP_HIP_H
#define PROMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct promp_ctx promp_ctx;

typedef struct promp_dims {
    int32_t n_tasks;            /* meta-tasks resident on this GPU (M_local)                       */
    int32_t n_tasks_global;     /* meta_batch_size over all ranks: the task-mean divides by this   */
    int32_t obs_dim;            /* O, 1..1024.  The fused kernels serve O <= 32 (hidden widths from {32,64}) and O <= 128
                                 * ((64,64) / (128,128)); everything else runs on the layer-by-layer kernels.
                                 * LinearFeatureBaseline's fit (2 O + 4 features) exists for O <= 480                        */
    int32_t act_dim;            /* A, 1..64 (fused kernels: A <= 8)                                */
    int32_t hidden1, hidden2;   /* the first two of hidden_sizes (policies/networks/mlp.py:5-62 takes any tuple).  Two tanh
                                 * layers of 1..128 units run on the fused kernels -- instantiated for {32,64} x {32,64}
                                 * (obs_dim <= 32) and (64,64) / (128,128), other widths zero-padded on the next of those;
                                 * wider layers (<= 256) and other depths run on the layer-by-layer kernels.  Every parameter
                                 * vector crosses this ABI in the caller's layout (promp_param_count floats,
                                 * policies/base.py:271-277 order)                                                          */
    int32_t num_inner_steps;    /* K = num_inner_grad_steps (>= 1)                                 */
    int32_t max_rows;           /* capacity: rows (env steps) per sampling step over local tasks   */
    int32_t max_paths;          /* capacity: paths per sampling step over local tasks              */
    /* ---- ABI 3 ---- */
    int32_t n_hidden;           /* len(hidden_sizes), 1..4; 0 means 2 (hidden1, hidden2)           */
    int32_t hidden3, hidden4;   /* widths of the third / fourth hidden layer (n_hidden >= 3 / 4)    */
    int32_t hidden_act;         /* hidden nonlinearity (policies/networks/mlp.py:47, policies/base.py:31): PROMP_ACT_TANH (0, the
                                 * reference's default and every run script's), PROMP_ACT_RELU, PROMP_ACT_IDENTITY (the reference's
                                 * hidden_nonlinearity=None: linear hidden layers).  Anything but tanh runs on the layer-by-layer kernels.
                                 * Bits 8..15: output_nonlinearity (policies/networks/mlp.py:53-60, 114-117: applied to the mean network's
                                 * last layer; None in every run script of the reference): PROMP_OUT_ACT_NONE (0), _TANH, _RELU, e.g.
                                 * PROMP_ACT_TANH | (PROMP_OUT_ACT_TANH << PROMP_OUT_ACT_SHIFT); layer-by-layer kernels as well */
} promp_dims;
enum { PROMP_ACT_TANH = 0, PROMP_ACT_RELU = 1, PROMP_ACT_IDENTITY = 2 };
enum { PROMP_OUT_ACT_NONE = 0, PROMP_OUT_ACT_TANH = 1, PROMP_OUT_ACT_RELU = 2, PROMP_OUT_ACT_SHIFT = 8 };

enum { PROMP_BASELINE_ZERO = 0, PROMP_BASELINE_LINEAR_FEATURE = 1, PROMP_BASELINE_LINEAR_TIME = 2 };
enum { PROMP_INNER_RATIO = 0,   /* -mean(ratio*adv)   meta_algos/pro_mp.py:59-65   */
       PROMP_INNER_LOGLIK = 1,  /* -mean(logpi*adv)   meta_algos/trpo_maml.py:58-62 */
       PROMP_INNER_DICE = 2     /* -mean(magic_box(cumsum logpi) * adjusted_reward * mask), meta_algos/dice_maml.py:39-45,245-258;
                                   needs promp_set_dice_rewards on every step; outer kind PROMP_OUTER_LOGLIK */ };
enum { PROMP_OUTER_CLIP = 0,    /* PPO clipped surrogate, meta_algos/pro_mp.py:141-145 */
       PROMP_OUTER_RATIO = 1,   /* unclipped,            meta_algos/trpo_maml.py:135    */
       PROMP_OUTER_KL = 2       /* mean KL(old || new) of the last step itself: the TRPO constraint
                                   (meta_algos/trpo_maml.py:133,147,158); its gradient through the
                                   adaptation feeds the finite-difference HVP of
                                   optimizers/conjugate_gradient_optimizer.py:59-89 */,
       PROMP_OUTER_LOGLIK = 3   /* -mean(logpi*adv) at the adapted parameters: VPG-MAML, meta_algos/vpg_maml.py:122-124 */ };

/* SampleProcessor.__init__ arguments (samplers/base.py:48-65) + baseline choice */
typedef struct promp_proc_opts {
    double discount;
    double gae_lambda;
    double reg_coeff;          /* LinearBaseline reg_coeff, baselines/linear_baseline.py:12,68 */
    int32_t normalize_adv;
    int32_t positive_adv;
    int32_t baseline_kind;     /* PROMP_BASELINE_* */
    int32_t reserved;          /* 0, or pad_length > 0: normalise / shift over each task's zero-padded [paths, pad_length] array
                                * (n = paths * pad_length, and a padded zero is a candidate for the minimum where the task has
                                * any padding), as the DiCE sample processor does (samplers/dice_sample_processor.py:165-191) */
} promp_proc_opts;

/* DiceSampleProcessor.__init__ arguments (samplers/dice_sample_processor.py:25-47) + baseline choices */
typedef struct promp_dice_opts {
    double  discount, gae_lambda, reg_coeff, return_reg_coeff;
    int32_t max_path_length, normalize_adv, positive_adv;
    int32_t baseline_kind;          /* PROMP_BASELINE_* : fitted on the discounted rewards */
    int32_t return_baseline_kind;   /* PROMP_BASELINE_* or -1: no GAE advantages */
    int32_t reserved;
} promp_dice_opts;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int promp_ctx_create(promp_ctx** out, int device_id, const promp_dims* dims);
void promp_ctx_destroy(promp_ctx* ctx);
const char* promp_last_error(void);
/* 3.  The version moves when an existing entry point changes its meaning or signature: 3 = promp_dims grew by n_hidden,
 * hidden3, hidden4 (hidden_sizes of any length 1..4; a v2 caller's two-layer struct is the same prefix, but the library reads the
 * new fields, so bindings must be rebuilt).  Entry points added since the first v2 header -- round 3: promp_set_reuse_adapt,
 * promp_begin_collection / promp_end_collection, promp_state_version, the two pass counters; round 4: promp_comm_fixed_order;
 * later: promp_set_train_step_sizes with promp_get_step_sizes / promp_get_step_size_grad / promp_{set,get}_step_size_adam_state
 * and promp_reduced_count; promp_set_outer_optimizer / promp_get_outer_optimizer / promp_get_grad_norm;
 * promp_process_samples_dice / promp_download_dice / promp_use_dice_advantages (and promp_proc_opts.reserved read as pad_length);
 * promp_rollout_point_family, promp_collect_point_family; promp_point_norm_set / promp_point_norm_get /
 * promp_collect_point_family_norm; promp_draw_point_starts / promp_rollout_point_family_dev / promp_collect_point_family_dev --
 * were additions and did not move it. */
int promp_abi_version(void);
/* Theta = O*H1+H1 + H1*H2+H2 + H2*A+A + A */
int promp_param_count(const promp_dims* dims);
/* LinearFeatureBaseline: 2*O+4 (baselines/linear_baseline.py:101-106); LinearTime: 4; Zero: 0 */
int promp_feature_dim(const promp_dims* dims, int baseline_kind);
int promp_sync(promp_ctx* ctx);

/* ---- trajectories ---------------------------------------------------------------------------
 * Upload one sampling step's paths (what MetaSampler.obtain_samples returns,
 * samplers/meta_sampler.py:59-137), flattened task-major, path-major, time-major:
 *   task_path_offsets [n_tasks+1] : paths of task i are [tpo[i], tpo[i+1])
 *   path_row_offsets  [n_paths+1] : rows of path p are  [pro[p], pro[p+1])   (ragged allowed)
 *   obs [rows,O], act [rows,A], rew [rows], old_mean [rows,A]  (agent_infos['mean'])
 *   old_log_std: [rows,A] when log_std_per_row != 0 (the reference's layout,
 *                policies/meta_gaussian_mlp_policy.py:135-136), else [n_tasks,A].
 * act / old_mean / old_log_std may be NULL when only process_samples is needed. */
int promp_upload_step(promp_ctx* ctx, int step, int n_paths,
                      const int32_t* task_path_offsets, const int32_t* path_row_offsets,
                      const float* obs, const float* act, const float* rew,
                      const float* old_mean, const float* old_log_std, int log_std_per_row);

/* Staged upload: the same arguments, but the copies go to the step's SECOND slab set on a copy stream and return at once;
 * promp_commit_step then makes that set the step's current one (a pointer swap on the host; the first launch that reads
 * it waits for the copies).  A trainer whose next batch exists while the current one is still being optimised (replayed
 * or asynchronously collected samples; bench.py's upload-inclusive number) hides the transfer under the compute:
 *     commit(0), commit(1), process_samples / adapt ..., stage(next 0), stage(next 1), optimize
 * Host arrays from promp_host_alloc (pinned) are read by DMA after the call returns: leave them untouched until
 * promp_stage_wait or the step's next commit + use; pageable arrays work too (the call then returns when they are read).
 * The reference has no counterpart (its feed_dict copies are synchronous, meta_algos/base.py:245-301). */
int promp_stage_step(promp_ctx* ctx, int step, int n_paths,
                     const int32_t* task_path_offsets, const int32_t* path_row_offsets,
                     const float* obs, const float* act, const float* rew,
                     const float* old_mean, const float* old_log_std, int log_std_per_row);
int promp_commit_step(promp_ctx* ctx, int step);
int promp_stage_wait(promp_ctx* ctx);
/* page-locked host memory for the arrays above (hipHostMalloc); NULL on failure */
void* promp_host_alloc(size_t bytes);
void promp_host_free(void* p);

/* ---- rows a1-a7: MetaSampleProcessor.process_samples (samplers/meta_sample_processor.py:8-49,
 * samplers/base.py:99-173, utils/utils.py:59-81, baselines/linear_baseline.py:17-106).
 * Computes on the device, per task: returns -> baseline fit -> GAE -> normalise; results stay
 * resident for promp_inner_adapt / promp_optimize.  Asynchronous. */
int promp_process_samples(promp_ctx* ctx, int step, const promp_proc_opts* opts);

/* Copy results of promp_process_samples to the host (any pointer may be NULL):
 *   returns [rows], advantages [rows] float32;  coeffs [n_tasks, feature_dim] float64
 *   (LinearBaseline._coeffs per task);  path_returns0 [n_paths] = returns[0] of each path,
 *   path_undiscounted [n_paths] = sum(rewards), path_reward_sumsq [n_paths] = sum(rewards^2)
 *   (float64; inputs of _log_path_stats, samplers/base.py:135-149, and of the adj_avg_rewards
 *   moments, samplers/meta_sample_processor.py:40-44). */
int promp_download_processed(promp_ctx* ctx, int step, float* returns, float* advantages, double* coeffs,
                             double* path_returns0, double* path_undiscounted, double* path_reward_sumsq);

/* float64 views of the same step: returns [rows] and the RAW (pre-normalisation) GAE advantages [rows], i.e. what the
 * reference stores back into every path dict (samplers/base.py:104,159).  Either pointer may be NULL. */
int promp_download_raw(promp_ctx* ctx, int step, double* returns64, double* raw_advantages64);

/* LinearBaseline.set_params / predict (baselines/linear_baseline.py:17-53) for the paths uploaded in `step`:
 * promp_set_coeffs installs coefficients [n_tasks, feature_dim(kind)] (float64); promp_predict_baseline evaluates
 * b = Phi . w per row with them -> baselines_out [rows] float64 (kind ZERO gives zeros). */
int promp_set_coeffs(promp_ctx* ctx, int step, int baseline_kind, const double* coeffs);
int promp_predict_baseline(promp_ctx* ctx, int step, int baseline_kind, double* baselines_out);

/* Use caller-provided advantages for a step instead of promp_process_samples' (float32 [rows]). */
int promp_set_advantages(promp_ctx* ctx, int step, const float* advantages);
/* DICE-MAML (meta_algos/dice_maml.py:39-45, 84-152, 245-258): the step's per-row rewards of the DiCE objective
 *   -mean_{p,t}( magic_box(sum_{t'<=t} logpi_{p,t'}) * adjusted_reward_{p,t} * mask_{p,t} ),
 * rewards [rows] float32 = adjusted_reward of every VALID row (path by path, as uploaded), already multiplied by
 * rows / (paths * max_path_length) of its task so that the slab mean equals the reference's mean over the zero-padded
 * [paths, max_path_length] array (samplers/dice_sample_processor.py:165-191).  Computes the suffix sums within each path
 * that weight the log-likelihood gradient and installs them as the step's advantages; PROMP_INNER_DICE additionally
 * couples the time steps of a path in the second-order term (two extra launches per R-operator pass). */
int promp_set_dice_rewards(promp_ctx* ctx, int step, const float* rewards);

/* DiceSampleProcessor._compute_samples_data (samplers/dice_sample_processor.py:96-191) on the step's resident slab, per task:
 * discounted rewards y_t = r_t gamma^t -> baseline fit on them -> adjusted = y - baseline -> normalise / shift over the
 * zero-padded [paths, max_path_length] array -> the DiCE rewards of the valid rows (x * rows / (paths * max_path_length)) and
 * their suffix sums.  Asynchronous, on the stream promp_process_samples would use.  Leaves the step as promp_set_dice_rewards
 * does (DiCE rewards, gradient weights as advantages) and processed.  With return_baseline_kind >= 0 the ordinary pipeline
 * (returns, fit, GAE, normalisation over the padded array) also runs on the step's rewards; its advantages, scaled the same way,
 * are kept beside the DiCE weights until promp_use_dice_advantages installs them as the step's advantages -- VPG_DICEMAML's
 * outer objective on the last step (meta_algos/vpg_dice_maml.py:46-49); the step is no DiCE data from then on.
 * Refused: max_path_length shorter than the step's longest path, an unknown kind, discount / gae_lambda outside [0,1], a step
 * without data. */
int promp_process_samples_dice(promp_ctx* ctx, int step, const promp_dice_opts* opts);
/* Results of promp_process_samples_dice (any pointer may be NULL; float64): adjusted / advantages [rows] = the normalised /
 * shifted values of the valid rows, BEFORE the rows / n scaling (the reference's samples hold them at the valid positions);
 * pad_adjusted / pad_advantages [n_tasks] = the value at every padded position of the task; coeffs / return_coeffs
 * [n_tasks, feature_dim(kind)]; per path: sum of rewards, sum of discounted rewards ("discounted return"), sum of rewards^2. */
int promp_download_dice(promp_ctx* ctx, int step, double* adjusted, double* advantages,
                        double* pad_adjusted, double* pad_advantages,
                        double* coeffs, double* return_coeffs,
                        double* path_undiscounted, double* path_discounted, double* path_reward_sumsq);
int promp_use_dice_advantages(promp_ctx* ctx, int step);

/* ---- parameters (rows a14: policies/base.py:173-203, 234-240, 262-286) ---------------------- */
int promp_set_theta(promp_ctx* ctx, const float* theta);                 /* [Theta] meta-parameters     */
int promp_get_theta(promp_ctx* ctx, float* theta);
int promp_set_step_sizes(promp_ctx* ctx, const float* step_sizes);       /* [Theta], base.py:303-313     */
/* The step sizes as they are now (base.py:203-211,303-313): what promp_set_step_sizes stored, the log_std entries zeroed under
 * learn_std = False, and -- trained -- moved by every Adam step since. */
int promp_get_step_sizes(promp_ctx* ctx, float* step_sizes);             /* [Theta]                      */
/* trainable_inner_step_size (base.py:203-211,303-313: the reference creates the step-size variables trainable and leaves them out
 * of its optimiser's var_list; here they are trained).  On: every gradient evaluation of the meta-objective (promp_meta_grad,
 * promp_optimize, promp_optimize_begin) also leaves d objective / d step sizes = mean over tasks of sum_k -lam_{k+1} * g_k, and
 * every Adam step (promp_adam_step and the two above) updates the step sizes together with theta: same beta_1, beta_2, epsilon,
 * bias-corrected learning rate and step count, slots of their own; entries of log_std under learn_std = False stay as they
 * are.  The one exchange per epoch then moves 2 Theta + K + 2 floats.  promp_constraint_hvp, promp_cg_solve and promp_eval_*
 * treat the step sizes as constants.  Costs (K + 1) x n_tasks x Theta floats of device memory, allocated when first switched on
 * (the sums a promp_meta_grad left for promp_reduced_get do not survive that).  Off (default): nothing is launched, allocated
 * or exchanged that a library without this entry point would not. */
int promp_set_train_step_sizes(promp_ctx* ctx, int on);
/* [Theta] the task-mean step-size gradient the last gradient evaluation left (base.py:203-211,303-313; entries that are not
 * trained report 0); needs promp_set_train_step_sizes(1) */
int promp_get_step_size_grad(promp_ctx* ctx, float* grad);
/* Adam slots of the step sizes (base.py:203-211,303-313; the step count is promp_set_adam_state's); need promp_set_train_step_sizes(1) */
int promp_set_step_size_adam_state(promp_ctx* ctx, const float* m, const float* v);
int promp_get_step_size_adam_state(promp_ctx* ctx, float* m, float* v);
/* GaussianMLPPolicy(learn_std=False) (policies/gaussian_mlp_policy.py:63-69: log_std_var created with trainable=False):
 * the trailing act_dim parameters are neither adapted by the inner step (their step sizes are forced to 0) nor updated
 * by Adam.  Default: learned. */
int promp_set_learn_std(promp_ctx* ctx, int learn_std);
/* GaussianMLPPolicy(min_std) (policies/gaussian_mlp_policy.py:31,35,71): log_std evaluated from the shared variables is
 * max(log_std_var, log min_std), gradient iff log_std_var >= log min_std (tf.maximum).  Default 1e-6. */
int promp_set_min_std(promp_ctx* ctx, float min_std);
/* Launch scheduling knobs (no reference counterpart; results are identical for every setting, -1 keeps a value):
 *   stage_overlap  != 0 (default): promp_process_samples of steps >= 1 is enqueued on a second stream, ordered behind the
 *                  last main-stream work on that step's slabs, and joined in front of the first launch that reads its
 *                  outputs -- it then runs under process_samples(0) + the inner step the host enqueued just before.
 *   fuse_min_tasks (default: never): from this many local tasks on, the Hessian-vector pass sums each task's partial rows
 *                  inside its own launch (last-arriving workgroup) instead of leaving it to the grid-wide reduction that
 *                  otherwise follows the launch (measured slower at every task count since that reduction was tuned). */
int promp_set_schedule(promp_ctx* ctx, int stage_overlap, int fuse_min_tasks);
/* Primal cache (no reference counterpart; hidden widths from {32, 64} only).  In one evaluation of the meta-gradient
 * (meta_algos/pro_mp.py:113-155) the inner gradient pass and the second-order pass of an adaptation step run at the same
 * parameters on the same slab; with the cache on, the former writes its hidden activations, means and first-layer
 * cotangents to HBM (4 (2 H1 + H2 + 8) bytes per row) and the latter reads them back instead of recomputing them.
 * Results agree with the recomputing path to float32 rounding (both evaluate the same tanh network; the two kernels
 * contract in different orders).  on = 1 always, 0 never, -1 (default) = always too since round 6 (the cache-reading pass is
 * less than half the recomputing one per tile and wins on 3-task shards as well; through round 5: from two rounds of 16-row
 * tiles per compute unit on). */
int promp_set_primal_cache(promp_ctx* ctx, int on);
/* The inner step and the first epoch of the optimisation that follows it evaluate the same pass.  MAMLAlgo._adapt
 * (meta_algos/base.py:217-242) runs the inner gradient step of every task from the meta-parameters; the first thing
 * ProMP.optimize_policy's graph (pro_mp.py:113-128) then evaluates is that very step again.  With reuse on (default),
 * promp_inner_adapt(step 0) from the pre-update state also leaves theta', the inner scalars and the primal cache where the
 * meta-objective's first evaluation looks for them, and that evaluation skips its first pass as long as nothing the pass reads
 * has changed since (meta-parameters, step-0 slab and advantages, step sizes, inner objective, min_std, learn_std; tracked by
 * version counters) and no log_std entry is below log(min_std) -- the one place where the two differ (raw log_std in the inner
 * step, policies/gaussian_mlp_policy.py:182; clipped in the graph's first step, :71,163).  The library knows the smallest
 * log_std entry from promp_set_theta or from the statistics the last optimisation published; otherwise it does not skip.
 * Bit-identical results either way.  promp_adapt_passes_skipped counts the skipped passes (for tests / logs). */
int promp_set_reuse_adapt(promp_ctx* ctx, int on);
long long promp_adapt_passes_skipped(promp_ctx* ctx);
/* R-operator passes of promp_constraint_hvp that read a step's primal cache instead of recomputing layers 1 and 2 (the
 * products of one conjugate-gradient solve run at the same parameters on the same slabs: the passes that refresh the chain
 * store, every pass of every product reads; governed by promp_set_primal_cache; for tests / logs) */
long long promp_constraint_hvp_cached_passes(promp_ctx* ctx);
/* A counter that moves whenever something an evaluation of the objectives depends on is replaced: the parameters (set /
 * Adam update), the inner step sizes, min_std / learn_std, a step's slabs or advantages.  Equal values before two evaluations
 * with the same arguments mean equal results: the host side uses it to answer TRPO's separate loss / constraint queries at
 * one parameter vector (optimizers/conjugate_gradient_optimizer.py:227-236 evaluates them one after the other) from one pass. */
long long promp_state_version(promp_ctx* ctx);
int promp_set_adam_state(promp_ctx* ctx, const float* m, const float* v, int64_t t);
int promp_get_adam_state(promp_ctx* ctx, float* m, float* v, int64_t* t);
/* MetaPolicy.switch_to_pre_update: replicate theta into every task's parameter slot */
int promp_switch_to_pre_update(promp_ctx* ctx);
/* MetaPolicy.update_task_parameters / policies_params_vals: per-task parameters [n_tasks,Theta] */
int promp_set_task_thetas(promp_ctx* ctx, const float* theta_tasks);
int promp_get_task_thetas(promp_ctx* ctx, float* theta_tasks);

/* ---- rows a8-a10: MAMLAlgo._adapt (meta_algos/base.py:217-242): for every local task
 *   theta_i <- theta_i - step_sizes * grad_theta L_i(theta_i)   on step `step`'s data,
 * explicit per-task parameters => raw log_std (policies/gaussian_mlp_policy.py:182).  Asynchronous. */
int promp_inner_adapt(promp_ctx* ctx, int step, int inner_kind);

/* ---- rollout-side inference: MetaGaussianMLPPolicy.get_actions
 * (policies/meta_gaussian_mlp_policy.py:99-157): mean network of every task's CURRENT parameters
 * (theta replicated after promp_switch_to_pre_update, adapted after promp_inner_adapt) on
 * obs [n_tasks, batch, O] -> mean_out [n_tasks, batch, A].  The Gaussian noise is added by the caller. */
int promp_policy_forward(promp_ctx* ctx, const float* obs, int batch, float* mean_out);

/* ---- rollouts that fill the step slab on the device -------------------------------
 * A device-side rollout lays the sampling step out as n_tasks * envs_per_task fixed-length paths:
 * path p of task i = rows [(i B + p) T, (i B + p + 1) T).
 *
 * (a) environments stepped by the host (MuJoCo ...): promp_begin_rollout once per sampling step, then per
 *     environment step t = 0 .. T-1 promp_policy_step: observations [n_tasks][B][O] in, actions [n_tasks][B][A] out.
 *     The device evaluates each task's mean network under its current parameters, draws the exploration noise
 *     (Philox4x32-10 keyed by `seed`, counter = slab row, Box-Muller), and writes observation, action and mean
 *     into the slab at row (task, env, t): what policies/meta_gaussian_mlp_policy.py:99-157 +
 *     samplers/meta_sampler.py:87-125 do with one sess.run and a Python loop per environment step.  The rewards
 *     follow once at the end (promp_set_rewards, float32 [rows]); promp_process_samples then needs no upload.
 *     clip_infos != 0: the log_std recorded for agent_infos is max(log_std, log 1e-6) (pre-update policy,
 *     policies/gaussian_mlp_policy.py:71); the noise scale always uses the raw value (:74).
 *     Every policy shape the context accepts is served (layer-by-layer shapes: one workgroup per environment). */
int promp_begin_rollout(promp_ctx* ctx, int step, int envs_per_task, int path_length);
/* (a') the same for environments whose episodes end early (samplers/meta_sampler.py:100-125: an environment that reports
 *     `done` is reset and keeps collecting; gym-style termination, e.g. envs/mujoco_envs/ant_rand_direc.py:32-46).  The slab
 *     cannot be laid out before the episode lengths are known, so promp_policy_step files the rows of vectorised step
 *     s = 0 .. max_steps-1 (its `t` argument) under (s, environment) in a staging area -- the Philox counter is that staging
 *     row, s * n_tasks * envs_per_task + environment -- and promp_end_collection copies the FINISHED episodes into the slab in
 *     path order once the host knows them: path p = steps [path_start[p], path_start[p] + path_len[p]) of environment
 *     path_env[p] (= task * envs_per_task + b); task_path_offsets [n_tasks + 1] as in promp_upload_step; rewards [rows] in path
 *     order.  Unfinished episodes are simply not listed (meta_sampler.py:114-125 drops them too).  2 * max_path_length - 1
 *     vectorised steps always suffice to finish n_tasks * envs_per_task * max_path_length environment steps. */
int promp_begin_collection(promp_ctx* ctx, int step, int envs_per_task, int max_steps);
int promp_end_collection(promp_ctx* ctx, int step, int n_paths, const int32_t* task_path_offsets, const int32_t* path_env,
                         const int32_t* path_start, const int32_t* path_len, const float* rewards);
int promp_policy_step(promp_ctx* ctx, int step, int t, const float* obs, uint64_t seed, int clip_infos, float* actions_out);
int promp_set_rewards(promp_ctx* ctx, int step, const float* rewards);
/* The same in the environment's float64: the reference scans float64 rewards (utils/utils.py:74-81 on the arrays the env
 * returned) and LinearBaseline.fit can be given arbitrary float64 targets; returns, GAE deltas and path statistics then
 * read these instead of the float32 copy (which is refreshed too, for promp_download_step). */
int promp_set_rewards_f64(promp_ctx* ctx, int step, const double* rewards);

/* (b) the 2-D point-mass meta-environment of BASELINE config 1, run_scripts/pro-mp_run_point_mass.py:
 *     normalize(MetaPointEnvCorner()) -- whole rollouts in one launch, one thread per environment:
 *       e = lb + (a + s)(ub - lb)/(2 s), clipped to [lb, ub]             envs/normalized_env.py:109-123: the normalize wrapper,
 *                                                                        s = normalization_scale (10), [lb, ub] = -+max_step;
 *                                                                        s = 0: bare environment, e = a
 *       state += clip(e, -max_step, max_step)                            envs/point_envs/point_env_2d_corner.py:37
 *       reward_type 0 dense -|s' - goal|, 1 dense_squared, 2 sparse      point_env_2d_corner.py:62-81
 *       no early termination                                             point_env_2d_corner.py:39
 *     goals [n_tasks][2], start [n_tasks][envs_per_task][2] (float64 like the NumPy environment);
 *     noise [n_tasks][envs_per_task][path_length][2] standard normals drawn by the caller, or NULL: drawn on the device
 *     from `seed` as in (a).  Asynchronous. */
typedef struct {
    double normalization_scale, max_step, sparse_radius;
    int32_t reward_type, clip_infos;
    uint64_t seed;
} promp_point_env_opts;
int promp_rollout_point_env(promp_ctx* ctx, int step, int envs_per_task, int path_length, const double* goals,
                            const double* start, const float* noise, const promp_point_env_opts* opts);

/* (b') the point-mass FAMILY: the reference's three fixed-horizon meta-environments with corner goals, the wrapper, the policy
 *     side, the noise and the slab exactly as in (b).  kind selects the environment; obs_dim of the context = state_dim:
 *       PROMP_POINT_CORNER   task_dim 2 (goal), state_dim 2: the environment of (b), same results bit for bit
 *       PROMP_POINT_WALLS    task_dim 6 (goal, gap_1, gap_2), state_dim 2        envs/point_envs/point_env_2d_walls.py:36-51, 71-83
 *           s' = p + clip(e, -max_step, max_step); the reward is taken on this s', before any wall acts:
 *           0 dense -|s' - goal|, 1 dense_squared, 2 sparse |p - goal| - |s' - goal| if |s' - goal| < sparse_radius.  Outside the
 *           radius the reference returns None, which its own normalize wrapper raises on and no sampler can sum: it is 0.0 here.
 *           if |p| < 1 and |s'| > 1:       s' <- s' / (|s'| + 1e-6)       unless |s' - gap_1| <= 1
 *           else if |p| < 2 and |s'| > 2:  s' <- s' / (0.5 |s'| + 1e-6)   unless |s' - gap_2| <= 1
 *           (every norm: squares, sum, root in float64; the reference's assertions are not reproduced)
 *       PROMP_POINT_MOMENTUM task_dim 2 (goal), state_dim 4 (position, velocity)  envs/point_envs/point_env_2d_momentum.py:36-42, 63-71
 *           v <- v + clip(e, -max_step, max_step); s' = s + v; observation (s', v);
 *           0 dense, 1 dense_squared, 2 sparse max(sparse_radius - |s' - goal|, 0)
 *     Neither environment ends an episode.  task_params [n_tasks][task_dim], start [n_tasks][envs_per_task][state_dim] (float64);
 *     noise as in (b).  An unknown kind, a task_dim that is not the kind's, a context whose obs_dim is not state_dim or whose
 *     act_dim is not 2 are refused.  Asynchronous. */
enum { PROMP_POINT_CORNER = 0, PROMP_POINT_WALLS = 1, PROMP_POINT_MOMENTUM = 2, PROMP_POINT_GOAL = 3 /* (b'') only */ };
typedef struct {
    int32_t kind;          /* PROMP_POINT_* */
    int32_t reward_type, clip_infos, task_dim;
    double normalization_scale, max_step, sparse_radius;
    uint64_t seed;
} promp_point_family_opts;
int promp_rollout_point_family(promp_ctx* ctx, int step, int envs_per_task, int path_length, const double* task_params,
                               const double* start, const float* noise, const promp_point_family_opts* opts);

/* (b'') the family with EARLY TERMINATION, collected without a host loop: what (a') does with one call per environment step, in a
 *     handful of launches (samplers/meta_sampler.py:87-130, samplers/vectorized_env_executor.py:25-52).  Every environment runs
 *     max_steps vectorised steps s; an episode ends when the environment says so or after max_path_length steps, and the
 *     environment then continues from start[s + 1][env], its next reset().  Step s is filed under the staging row
 *     s * n_envs + env of (a') -- the Philox counter when noise is NULL -- with its reward.  Collection stops at s*, the first step
 *     after which total_samples steps belong to finished episodes; all episodes that end at s* count (the rows may exceed
 *     total_samples, as in the reference's loop), episodes still running are dropped.  The finished episodes are listed per task
 *     in the reference's order -- by the step they end at, then by environment -- and copied into the slab with their rewards.
 *       kind PROMP_POINT_CORNER / WALLS / MOMENTUM: the environments of (b'); their episodes end by max_path_length alone
 *       kind PROMP_POINT_GOAL  task_dim 2 (goal), state_dim 2      envs/point_envs/point_env_2d.py, point_env_2d_v2.py
 *           s' = s + clip(e, -max_step, max_step); reward -|s' - goal|; done = |s'_0| < done_radius and |s'_1| < done_radius,
 *           the box around the ORIGIN (as both reference classes have it).  point_env_2d.py is goal = (0, 0).  reward_type and
 *           sparse_radius are not read.
 *     task_params [n_tasks][task_dim]; start [max_steps][n_envs][state_dim]: row 0 the initial states, row s + 1 the state an
 *     environment whose episode ends at step s continues from (n_envs = n_tasks * envs_per_task, environment = task *
 *     envs_per_task + b); noise [max_steps][n_envs][2] or NULL.
 *     Out: n_paths, n_steps = s* + 1, task_path_offsets [n_tasks + 1], path_env / path_start / path_len [max_paths of the context]
 *     (the first n_paths are written): the arguments promp_end_collection takes.  The step is left as promp_end_collection leaves
 *     it.  Refused, with no layout installed: max_steps too small to reach total_samples; more rows than max_rows or more paths
 *     than max_paths; a task without a finished episode; max_path_length < 1; and what (b') refuses.  Synchronous. */
typedef struct {
    promp_point_family_opts env;      /* kind 0..3, clip_infos, seed, the wrapper's scale, the action box */
    double  done_radius;              /* PROMP_POINT_GOAL: 0.01 */
    int32_t max_path_length, max_steps;
    int64_t total_samples;
} promp_point_collect_opts;
int promp_collect_point_family(promp_ctx* ctx, int step, int envs_per_task, const double* task_params, const double* start,
                               const float* noise, const promp_point_collect_opts* opts, int32_t* n_paths, int32_t* n_steps,
                               int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len);

/* (b''') (b'') under the normalize wrapper's RUNNING observation / reward normalisation: normalize(env, normalize_obs=True,
 *     normalize_reward=True) (envs/normalized_env.py:73-123; the executor and the sampler loop that drive it:
 *     samplers/vectorized_env_executor.py:25-75, samplers/meta_sampler.py:87-130).  Every environment e = task * envs_per_task + b
 *     owns one wrapper state of 2 state_dim + 2 float64: obs_mean [state_dim], obs_var [state_dim], rew_mean, rew_var (a fresh
 *     wrapper: 0 / 1 / 0 / 1).  It lives in the context across calls -- the K + 1 sampling steps of an iteration and the iterations --
 *     and no task change touches it.  One update with sample x and step size alpha, float64, every product rounded on its own:
 *       mean <- (1 - alpha) mean + alpha x;   var <- (1 - alpha) var + alpha (x - mean)^2        (the NEW mean)
 *     Per vectorised step s of environment e:
 *       the call's first reset(): start[0][e] updates the obs moments                            normalized_env.py:91-96
 *       the policy is handed float32((x - mean) / (sqrt(var) + 1e-8)) (normalize_obs 0: float32(x)); the bare environment steps
 *         on its RAW state, `done` and every reward formula see raw values only                   normalized_env.py:109-118
 *       normalize_obs: the raw next observation, the terminal one of an episode included, updates the obs moments    :119-120
 *       normalize_reward: the raw reward r updates the reward moments; stored is float32(r / (sqrt(rew_var) + 1e-8))  :121-122
 *       the episode ends: reset() at once, start[s + 1][e] updates the obs moments               vectorized_env_executor.py:45-52
 *         -- at the stop step s* too, whose fresh observation nobody uses.
 *     The state the call leaves is the state after step s*; the steps the device runs beyond s* leave no trace in it, and a
 *     refused call leaves it bit for bit as it was.  start is [max_steps + 1][n_envs][state_dim].
 *   promp_point_norm_set  allocates and fills the context's state: moments [n_envs][2 state_dim + 2], per environment obs_mean,
 *     obs_var, rew_mean, rew_var.  promp_point_norm_get reads it back (refused when none was set, or for other sizes).
 *   promp_collect_point_family_norm  promp_collect_point_family's arguments plus the options.  With both flags 0 it IS
 *     promp_collect_point_family on the first max_steps rows of start, bit for bit, and the state is not read or written.
 *     Refused by name: a flag set but no state set, or one set for another n_envs / state_dim; an alpha outside [0, 1] or not finite;
 *     everything promp_collect_point_family refuses.  Synchronous. */
typedef struct {
    int32_t normalize_obs, normalize_reward;
    double  obs_alpha, reward_alpha;
} promp_point_norm_opts;
int promp_point_norm_set(promp_ctx* ctx, int n_envs, int state_dim, const double* moments);
int promp_point_norm_get(promp_ctx* ctx, int n_envs, int state_dim, double* moments);
int promp_collect_point_family_norm(promp_ctx* ctx, int step, int envs_per_task, const double* task_params, const double* start,
                                    const float* noise, const promp_point_collect_opts* opts, const promp_point_norm_opts* norm,
                                    int32_t* n_paths, int32_t* n_steps, int32_t* task_path_offsets, int32_t* path_env,
                                    int32_t* path_start, int32_t* path_len);

/* (b'''') START STATES DRAWN ON THE DEVICE: (b'), (b'') and (b''') without a start table.  What replaces the table is the reset() of
 *     the reference's classes -- np.random.uniform over a box, or zeros:
 *       envs/point_envs/point_env_2d_corner.py:50        uniform(-0.2, 0.2, 2)
 *       envs/point_envs/point_env_2d_walls.py:60         uniform(-0.2, 0.2, 2)
 *       envs/point_envs/point_env_2d_momentum.py:51-52   uniform(-0.2, 0.2, 2) and a velocity uniform(-0.1, 0.1, 2)
 *       envs/point_envs/point_env_2d.py:37               uniform(-2, 2, 2)
 *       envs/point_envs/point_env_2d_v2.py:40            zeros(2)                 (lo = hi = 0)
 *     Coordinates 2 p and 2 p + 1 of the reset() filed under start-table row r come from one Philox4x32-10 block:
 *       counter (lo32(r), hi32(r), 0x80000000 | p, stream), key (lo32(seed), hi32(seed))
 *     r = s * n_envs + env, s the row of the table of (b'') / (b''') -- row 0 the initial states, row s + 1 the state an environment
 *     continues from after an episode that ends at step s; under (b''') the row behind the last step, s = max_steps, is drawn like
 *     any other --; the fixed-horizon rollouts of (b') have r = env.  stream is the step slot, as for the noise of (a).  The high bit
 *     of counter word 2 keeps these blocks apart from the action-noise blocks, whose word 2 is an action pair below 32, so one seed
 *     may serve both.  Words (x, y) give coordinate 2 p, words (z, w) coordinate 2 p + 1:
 *       u = ((a >> 5) * 2^26 + (b >> 6)) / 2^53, a float64 in [0, 1);  value = lo[k] + (hi[k] - lo[k]) * u, every operation rounded
 *       on its own (no fused multiply-add), so lo[k] == hi[k] yields exactly lo[k].
 *     The stream is a function of (seed, step slot, table row, environment) and of nothing else -- no launch geometry, no kernel.
 *   promp_draw_point_starts  out [n_rows][n_envs][state_dim] (host): the table the other two calls behave as if they had been
 *     handed.  state_dim 2 or 4.  Synchronous.
 *   promp_rollout_point_family_dev / promp_collect_point_family_dev  the arguments of promp_rollout_point_family /
 *     promp_collect_point_family_norm with `starts` in the place of `start`; norm may be NULL (the plain collection).  Results are
 *     those of the table entry points on promp_draw_point_starts' table, bit for bit.  noise is host noise or NULL, independently of
 *     the starts (opts->seed keys the noise, starts->seed the start states).  No start table is reserved or uploaded: a call uploads
 *     the task parameters and, if given, the noise.  Refused by name, with nothing installed and, under norm, the moments bit for
 *     bit as they were: starts NULL; lo[k] > hi[k] or a bound that is not finite for some k < state_dim; everything the table
 *     entry points refuse. */
typedef struct {
    double   lo[4], hi[4];    /* coordinate k < state_dim of every reset(): lo[k] + (hi[k] - lo[k]) u, u in [0, 1) */
    uint64_t seed;
} promp_point_start_opts;
int promp_draw_point_starts(promp_ctx* ctx, int step, int n_rows, int n_envs, int state_dim, const promp_point_start_opts* starts,
                            double* out);
int promp_rollout_point_family_dev(promp_ctx* ctx, int step, int envs_per_task, int path_length, const double* task_params,
                                   const promp_point_start_opts* starts, const float* noise, const promp_point_family_opts* opts);
int promp_collect_point_family_dev(promp_ctx* ctx, int step, int envs_per_task, const double* task_params,
                                   const promp_point_start_opts* starts, const float* noise, const promp_point_collect_opts* opts,
                                   const promp_point_norm_opts* norm /* or NULL */, int32_t* n_paths, int32_t* n_steps,
                                   int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len);

/* (c) ENVIRONMENTS THAT LIVE ON THE DEVICE: (a) and (a') for a simulator that runs on the same GPU (a vectorised environment written
 *     with an array library on ROCm, a kernel of the caller's).  Observations, actions, rewards and `done` flags never visit the
 *     host, and no call of the per-step loop synchronises.
 *     ORDERING.  Every entry point below that reads or writes caller device memory takes `producer_stream`: the hipStream_t the
 *     caller's simulator enqueues on, 0 = the null stream.  At entry the context's stream waits for an event recorded on the
 *     producer stream; before returning, the producer stream waits for an event recorded on the context's stream.  So the call
 *     sees everything the producer enqueued before it, and the caller may overwrite its buffers right after the call and read the
 *     outputs in stream order, without synchronising.  Two events per context, timing disabled; no stream is created.
 *     POINTERS.  promp_check_device_pointer returns 0 when the GPU can read through the pointer (device memory, page-locked host
 *     memory), -1 with a message otherwise (NULL, pageable host memory); it launches nothing.  Every *_dev entry point applies it
 *     to every caller pointer before it enqueues anything: a host pointer never reaches a kernel.
 *   promp_policy_step_dev  promp_policy_step with d_obs [n_tasks][B][O] and d_actions [n_tasks][B][A] in device memory, after
 *     promp_begin_rollout or promp_begin_collection: no copy, no synchronisation.  The same kernels file the same slab / staging
 *     rows under the same Philox counter and stream word: for equal observations and seed, rows and actions are bit for bit those
 *     of promp_policy_step.  Asynchronous.
 *   promp_file_step_dev  files the outcome of vectorised step s, one thread per environment (environment = task * B + b).  The
 *     context keeps a per-environment episode length, zeroed by s = 0:
 *       len = ep_len[env] + 1;  end = (d_done && d_done[env]) || len == max_path_length
 *       staged reward (s, env) = d_rewards[env];  end_len (s, env) = end ? len : 0;  ep_len[env] = end ? 0 : len
 *       d_ended_out[env] = end
 *     -- what k_point_collect files for its own environments.  The simulator must reset the environments flagged in d_ended_out
 *     before the next policy step.  d_done and d_ended_out may each be NULL.  After promp_begin_rollout (fixed horizon) the reward
 *     goes straight to slab row env * T + s, d_done is not read and `end` is s == T - 1.  Steps are filed in order 0, 1, 2, ...,
 *     once each, each after its policy step; anything else is refused by name from host-side counters before any launch.
 *     Asynchronous.
 *   promp_collection_progress  the stop rule of (b'') over the steps filed so far: *stop_step = s*, the first step after which
 *     total_samples steps lie in finished episodes, with *finished_rows their number at s*; -1 (and 0): not reached yet.
 *     Synchronous.
 *   promp_end_collection_dev  the tail of (b'') over the filed steps: stop step, path tables (count, offsets, write), the same
 *     validations and refusals, then the finished episodes and their staged rewards go to the slab.  Out: as
 *     promp_collect_point_family.  A refused call installs nothing and leaves the collection open; when total_samples has not been
 *     reached, more steps can be filed and the call repeated.  Steps filed beyond s* are ignored.  Synchronous.
 *   promp_upload_step_dev  promp_upload_step with obs, act, rew, old_mean and old_log_std in device memory (the two offset tables
 *     stay on the host): device-to-device copies; the step is then in every respect what promp_upload_step leaves.
 *   promp_dev_alloc / promp_dev_free / promp_dev_upload / promp_dev_download  hipMalloc, hipFree and synchronous copies on the
 *     context's device and stream, for callers without a GPU array library.
 *   Not here: running normalisation of an external environment, env_infos, float64 rewards, sharding one environment over ranks. */
int promp_check_device_pointer(const void* p);
void* promp_dev_alloc(promp_ctx* ctx, size_t bytes);
void promp_dev_free(promp_ctx* ctx, void* p);
int promp_dev_upload(promp_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
int promp_dev_download(promp_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);
int promp_policy_step_dev(promp_ctx* ctx, int step, int t, const float* d_obs, uint64_t seed, int clip_infos, float* d_actions,
                          void* producer_stream);
int promp_file_step_dev(promp_ctx* ctx, int step, int s, const float* d_rewards, const uint8_t* d_done, int max_path_length,
                        uint8_t* d_ended_out, void* producer_stream);
int promp_collection_progress(promp_ctx* ctx, int step, int64_t total_samples, int32_t* stop_step, int64_t* finished_rows);
int promp_end_collection_dev(promp_ctx* ctx, int step, int64_t total_samples, int32_t* n_paths, int32_t* n_steps,
                             int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len);
int promp_upload_step_dev(promp_ctx* ctx, int step, int n_paths, const int32_t* task_path_offsets, const int32_t* path_row_offsets,
                          const float* obs, const float* act, const float* rew, const float* old_mean, const float* old_log_std,
                          int log_std_per_row, void* producer_stream);

/* Step slab back on the host (any pointer may be NULL): obs [rows][O], act [rows][A], rew [rows],
 * old_mean [rows][A], old_log_std [rows | n_tasks][A] as uploaded / produced by a device rollout. */
int promp_download_step(promp_ctx* ctx, int step, float* obs, float* act, float* rew, float* old_mean, float* old_log_std);

/* ---- rows a11-a13 ---------------------------------------------------------------------------
 * One evaluation of the ProMP meta-objective (meta_algos/pro_mp.py:67-163) and of its exact
 * gradient (what tf.gradients yields through meta_algos/base.py:206, i.e. including the
 * second-order MAML term), over steps 0..K of resident data, reduced over local tasks and, when a
 * communicator is attached, all-reduced over ranks; leaves the task-MEAN gradient on the device.
 *   stats_out [K+2] = { loss, inner_kl[0..K-1], outer_kl };  grad_out [Theta] (may be NULL). */
int promp_meta_grad(promp_ctx* ctx, float clip_eps, const float* inner_kl_coeff, int inner_kind, int outer_kind,
                    float* grad_out, float* stats_out);
/* ConjugateGradientOptimizer's Hessian-vector product of the constraint (optimizers/conjugate_gradient_optimizer.py:59-89
 * builds it by finite differences of the constraint gradient, hvp_approach=FiniteDifferenceHvp; SURVEY 8f row 2 asks
 * for the exact one): out [Theta] = H v, H = Hessian wrt theta of mean_i KL(pi_old || pi_{theta'_i(theta)}) on the last
 * step's samples (trpo_maml.py:146-158), through the K inner steps (Gauss-Newton form J^T H_KL J: exact where the old
 * distribution is the adapted policy's, i.e. at the parameters TRPO evaluates it).  The mean is over the GLOBAL
 * meta-batch (all-reduce when a communicator is attached).  refresh_chain != 0 recomputes the adapted parameters
 * theta_k from the current theta first (needed once per theta).  No reg_coeff term: the caller adds reg_coeff * v.
 * Every supported policy shape (register-chained and cooperative kernels); the register-chained ones keep primal caches
 * over the products of one solve (promp_set_primal_cache, promp_constraint_hvp_cached_passes). */
int promp_constraint_hvp(promp_ctx* ctx, int inner_kind, const float* v, int refresh_chain, float* out);
/* ConjugateGradientOptimizer's whole solve on the device (optimizers/conjugate_gradient_optimizer.py:325-354 conjugate_gradients();
 * :59-104 FiniteDifferenceHvp.Hx / build_eval -- the product x -> (H + reg_coeff I) x of the constraint; :259-264 the solve inside
 * optimize() and the closing product that sizes the step): cg_iters conjugate-gradient iterations on (H + reg_coeff I) x = b from x = 0, then x . (H + reg_coeff I) x.
 *   hvp_mode 0  H v = (grad c(theta + eps v) - grad c(theta - eps v)) / (2 eps)   (the reference's default: symmetric, eps 1e-5)
 *            1  H v = (grad c(theta + eps v) - grad c(theta)) / eps
 *            2  the exact product of promp_constraint_hvp (eps unused)
 * with grad c the gradient of the mean outer KL through the adaptation (promp_meta_grad with PROMP_OUTER_KL).  Same arithmetic
 * as the host loop over promp_set_theta / promp_meta_grad (float32 vectors; the dot products are summed in float64 in a fixed
 * order), but nothing crosses to the host between the products: 2 cg_iters + 2 gradient evaluations enqueued back to back, one
 * synchronisation at the end.  The iteration stops updating once r.r < residual_tol (1e-10 in the reference).  The parameters
 * are back at theta when the call returns.  b [Theta] = the loss gradient; x_out [Theta]; *xhx_out = x . (H + reg_coeff I) x. */
int promp_cg_solve(promp_ctx* ctx, int inner_kind, const float* b, int cg_iters, float reg_coeff, float eps, int hvp_mode,
                   float residual_tol, float* x_out, double* xhx_out);
/* Subsampled constraint products (ConjugateGradientOptimizer's subsample_factor, as in rllab's TRPO: the products x -> H x of
 * the solve and the closing x . H x see a subset of the paths; the loss, its gradient and the line search see the whole batch).
 * promp_set_step_selection: path_idx [n_sel] = indices into the step's paths, strictly increasing, at least one path of every
 * task; n_sel = 0 or path_idx = NULL clears the step's selection.  A malformed selection is refused with a message and nothing
 * is written.  The selected paths' rows (observations, actions, advantages, old means and log_std) are copied into a compact
 * slab laid out exactly as promp_upload_step would lay out an upload of those paths alone, on first use and again whenever the
 * step's data has moved (promp_process_samples / promp_set_advantages after the selection are seen); whatever replaces the
 * step's layout (promp_upload_step, promp_commit_step, the rollout entry points, promp_end_collection) clears the selection.
 * The constraint on a selection is the same function on fewer paths: the inner adaptation runs on the selected paths of steps
 * 0..K-1, the KL mean over those of step K, the old distributions are the stored ones.  Its exact product J_S^T H_KL J_S is
 * positive semi-definite but no longer the full Hessian: the adapted parameters on a subsample are not the ones step K was
 * sampled with, so the dropped third-order term is not zero.
 *   promp_cg_solve            runs every product (all three modes) on the selections when EVERY step has one; refuses when only
 *                             some have.  Without any, it is bit for bit what it was.
 *   promp_use_selection(on)   promp_meta_grad with PROMP_OUTER_KL and promp_constraint_hvp evaluate on the selections (every
 *                             step must have one) until switched off: the host loop's and external collectives' way in.
 *   promp_step_selection      the number of selected paths of a step, 0: none.
 * The evaluations on selections keep a chain of adapted parameters, inner scalars and a primal-cache record of their own: what
 * promp_inner_adapt and the last full-batch product left behind stays valid.  PROMP_INNER_DICE is refused on a selection. */
int promp_set_step_selection(promp_ctx* ctx, int step, int n_sel, const int32_t* path_idx);
int promp_step_selection(promp_ctx* ctx, int step);
int promp_use_selection(promp_ctx* ctx, int on);
/* The outer optimiser's step on theta with the gradient left by promp_meta_grad: tf.train.AdamOptimizer
 * (optimizers/maml_first_order_optimizer.py:24,64; b1=.9 b2=.999 eps=1e-8, bias-corrected lr) unless promp_set_outer_optimizer
 * asked for another rule or other arguments. */
int promp_adam_step(promp_ctx* ctx, float learning_rate);
/* The update rule of every stepping entry point (promp_adam_step, promp_optimize[_begin], promp_optimize_minibatch[_begin]):
 * MAMLFirstOrderOptimizer's tf_optimizer_cls(**tf_optimizer_args) (optimizers/maml_first_order_optimizer.py:22-38), TF1 semantics.
 * g is the task-mean gradient (clipped when clipping is on), lr the call's learning rate, t the step count, which advances
 * under every rule:
 *   PROMP_OUTER_ADAM      args = {beta1, beta2, epsilon, -}   slots m, v
 *       lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) (host, double);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *       theta -= lr_t m / (sqrt(v) + epsilon).  Default {0.9, 0.999, 1e-8}; an argument equal to a default's float32 value IS the
 *       default (lr_t then uses the double constants 0.9 / 0.999 it always has).
 *   PROMP_OUTER_SGD       args unused, no slots                theta -= lr g
 *   PROMP_OUTER_MOMENTUM  args = {momentum, use_nesterov (0 / 1), -, -}   slot a, kept where Adam keeps m
 *       a = momentum a + g;  theta -= lr a;  with use_nesterov:  theta -= lr (g + momentum a), a the new one.
 * args = NULL: the rule's defaults (momentum 0, no Nesterov step).  Refused with a message, nothing changed: an unknown rule,
 * beta or momentum outside [0, 1), epsilon <= 0, a negative or non-finite max_grad_norm.  Entries that are not trained
 * (learn_std = False) are masked under every rule; trained step sizes take the same rule and arguments with slots of their own.
 * Setting a DIFFERENT rule zeroes m, v, the step count and the step sizes' slots; the same rule with new arguments keeps them.
 * promp_set_adam_state / promp_get_adam_state work under every rule (a slot a rule does not use is carried along).
 *
 * max_grad_norm = c > 0: the task-mean gradient is scaled by the global norm before the rule sees it, n = sqrt(sum_j g_j^2)
 * over the trained entries of theta and, when they are trained, of the step sizes; scale = n > c ? c / n : 1 -- exactly 1 when
 * the clip is not active, which tf.clip_by_global_norm's c * min(1 / n, 1 / c) equals up to the last bit only; a non-finite n
 * gives non-finite updates, as there.  The norm is the GLOBAL meta-batch's (taken behind the exchange), summed in float64 in one
 * fixed order by every workgroup of the stepping launch; what promp_meta_grad hands out stays the unclipped gradient.  With
 * clipping on, a step is always sums -> [exchange] -> mean + step (one dependent launch more per epoch on a single rank).
 * 0 (default): off.  With nothing set, every launch and argument is that of a library without this entry point. */
enum { PROMP_OUTER_ADAM = 0, PROMP_OUTER_SGD = 1, PROMP_OUTER_MOMENTUM = 2 };
int promp_set_outer_optimizer(promp_ctx* ctx, int rule, const float args[4], float max_grad_norm);
int promp_get_outer_optimizer(promp_ctx* ctx, int* rule, float args[4], float* max_grad_norm);
/* the unclipped global norm n of the last gradient a step was taken on; refused while clipping is off or before the first step */
int promp_get_grad_norm(promp_ctx* ctx, float* out);
/* ProMP.optimize_policy's numerical core (meta_algos/pro_mp.py:165-199 +
 * optimizers/maml_first_order_optimizer.py:82-115,146-163): num_epochs x (meta_grad, Adam), then
 * compute_stats.  loss_before = loss of the first epoch; stats_after [K+2] as in promp_meta_grad.
 * Everything is enqueued back-to-back; one synchronisation at the end. */
int promp_optimize(promp_ctx* ctx, int num_epochs, float learning_rate, float clip_eps,
                   const float* inner_kl_coeff, int inner_kind, int outer_kind,
                   float* loss_before, float* stats_after);
/* The same in two halves.  promp_optimize_begin enqueues everything (epochs, compute_stats, an asynchronous copy of
 * the statistics to page-locked memory) and returns without waiting; promp_optimize_end waits for that copy and hands
 * out loss_before / stats_after.  Between the two the caller may enqueue work that does not depend on the statistics --
 * Trainer.train's next process_samples / _adapt (meta_trainer.py:105-116); the KL-coefficient rule (pro_mp.py:201-214)
 * needs them only in front of the next optimize_policy.  One optimisation may be pending at a time. */
int promp_optimize_begin(promp_ctx* ctx, int num_epochs, float learning_rate, float clip_eps,
                         const float* inner_kl_coeff, int inner_kind, int outer_kind);
int promp_optimize_end(promp_ctx* ctx, float* loss_before, float* stats_after);
/* Minibatched Adam epochs: what the reference's `num_minibatches` promises and never implements ("number of mini-batches for
 * performing the gradient step. The mini-batch size is batch size//num_minibatches": optimizers/maml_first_order_optimizer.py:
 * 16-17; stored at :41 as "# Unused"; ":97-99  # Todo: reimplement minibatches").  An epoch is num_minibatches Adam steps instead
 * of one.  assign [num_epochs][sum_k n_paths_k] (int32, steps 0..K one behind the other) names, for every epoch and sampling
 * step, the minibatch in [0, num_minibatches) of each path; every task must keep at least one path of every step in every
 * minibatch.  Minibatch j of an epoch is the meta-objective on share j of every task at every step -- the inner adaptation on
 * share j of steps 0..K-1, the outer objective, the outer KL and the inner-KL penalty on share j, the means over the share's
 * rows, the mean over all tasks: the same function on fewer paths, as a selection (promp_set_step_selection) is.  Advantages, old
 * means and old log_std are the stored ones; nothing is renormalised per minibatch.  Per (epoch, step) ONE launch deals the
 * step's paths to the minibatches' compact slabs, each laid out exactly as promp_upload_step would lay out an upload of those
 * paths alone; the Adam steps of an epoch follow in the order j = 0 .. num_minibatches - 1 (adam_t advances by num_minibatches
 * per epoch; trained step sizes step along).  loss_before is the WHOLE batch's objective before the first step (one extra
 * forward-only evaluation), stats_after the whole batch's behind the last: the statistics never see a minibatch quantity.
 * num_minibatches = 1 is promp_optimize_begin itself (assign is not read).  Everything is validated before anything is
 * enqueued, and nothing waits for the device between the first enqueue and the return; promp_optimize_end collects.  What the
 * call leaves behind (the chain of adapted parameters, the constraint products' caches, the selections) is what promp_optimize
 * leaves: the minibatch evaluations keep a chain, inner scalars and caches of their own.  Refused: PROMP_INNER_DICE and steps
 * that carry DiCE rewards (the coupling rows are not among the copies), a sharded context without a communicator, a pending
 * optimisation.  With a communicator every Adam step has its one exchange, as an epoch of promp_optimize has. */
int promp_optimize_minibatch_begin(promp_ctx* ctx, int num_epochs, int num_minibatches, const int32_t* assign, float learning_rate,
                                   float clip_eps, const float* inner_kl_coeff, int inner_kind, int outer_kind);
int promp_optimize_minibatch(promp_ctx* ctx, int num_epochs, int num_minibatches, const int32_t* assign, float learning_rate,
                             float clip_eps, const float* inner_kl_coeff, int inner_kind, int outer_kind, float* loss_before,
                             float* stats_after);

/* ---- multi-GPU: task-sharded data parallelism, one process per GPU, RCCL over xGMI.
 * The only exchange on the path is the task-mean of the meta-objective / its gradient
 * (meta_algos/pro_mp.py:122,151,155): ONE all-reduce of [Theta+K+2] floats per epoch. */
int promp_comm_unique_id(void* id_out, size_t id_bytes);                  /* rank 0; 128 bytes  */
int promp_comm_init(promp_ctx* ctx, int rank, int nranks, const void* id, size_t id_bytes);
int promp_allreduce_f64(promp_ctx* ctx, double* host_buf, int n, int op /*0 sum, 1 max*/);
/* Hand the communicator of `src` over to `dst` (same device): a context that is re-created with more capacity
 * keeps its communicator instead of running a new rendezvous -- ranks with ragged batches regrow at different
 * times, a rendezvous per regrow would deadlock.  `src` is left single-rank. */
int promp_comm_move(promp_ctx* dst, promp_ctx* src);
/* Take the several-rank launch sequence (per-rank sums -> [all-reduce] -> mean + Adam as separate launches) even on
 * one rank; numerically identical to the fused single-rank launch (the parity tests assert bitwise equality). */
int promp_comm_split_path(promp_ctx* ctx, int on);
/* What the attached communicator says about itself (ncclCommCount, ncclCommUserRank; 1 / 0 without one), whether the exchange is
 * the fixed-order one, and the PCI bus id of the context's device: evidence for a benchmark line that N ranks on N distinct GPUs
 * took part (meta_algos/pro_mp.py:122,151,155 is the mean the exchange computes).  Any output may be NULL. */
int promp_comm_info(promp_ctx* ctx, int32_t* nranks, int32_t* rank, int32_t* fixed_order, char* bus_id_out, size_t bus_id_bytes);
/* The exchange as ncclAllGather + a sum in rank order (0, 1, ...) on every rank instead of ncclAllReduce: the replicas'
 * parameters are bitwise identical by construction -- not by the grace of RCCL choosing the same reduction order on every
 * rank -- and equal to one process adding the ranks' shards in that order.  The buffer is ~6 k floats:
 * the gather moves nranks x 24 KB, latency as the all-reduce's.  Set it the same on every rank; default off. */
int promp_comm_fixed_order(promp_ctx* ctx, int on);
/* The buffer the all-reduce acts on, [Theta + K + 2] floats = { grad sums | J sum | inner-KL sums [K] | outer-KL sum }
 * over the LOCAL tasks after promp_meta_grad (when n_tasks_global > n_tasks and no communicator is attached, the
 * exchange is the caller's: get, reduce over ranks with any collective, set, then promp_adam_step -- which divides by
 * n_tasks_global). */
int promp_reduced_get(promp_ctx* ctx, float* out);
int promp_reduced_set(promp_ctx* ctx, const float* in);
/* The length the two above act on: Theta + K + 2, and with trainable step sizes (base.py:203-211,303-313) 2 Theta + K + 2 --
 * the task sums of the step-size gradient follow the scalars. */
int promp_reduced_count(promp_ctx* ctx);

/* ---- evaluation hooks used by the parity tests and by alternative optimizers (TRPO-MAML's
 * conjugate-gradient loop calls these per evaluation): per-task objective, mean-KL and their
 * gradient at the CURRENT per-task parameters on step `step`'s data.
 *   kind: 0 ratio surrogate, 1 clipped surrogate, 2 log-likelihood, 3 mean KL(old||new)
 *   grads_out [n_tasks,Theta], loss_out [n_tasks], kl_out [n_tasks] (any may be NULL). */
int promp_eval_loss_grad(promp_ctx* ctx, int step, int kind, float clip_eps, int clip_log_std,
                         float* grads_out, float* loss_out, float* kl_out);
/* per task: out_i = -H_i v_i + kl_weight * grad KL_i, H_i = Hessian of the inner objective at the
 * current per-task parameters on step `step`'s data; v [n_tasks,Theta]; out [n_tasks,Theta]. */
int promp_eval_hvp(promp_ctx* ctx, int step, int inner_kind, int clip_log_std, float kl_weight,
                   const float* v, float* out);

/* ---- measurement: HIP-event timing of the pass kernels on the context's stream ------------- */
enum { PROMP_KERNEL_FWD_BWD = 0, PROMP_KERNEL_HVP = 1, PROMP_KERNEL_GRAM = 2, PROMP_KERNEL_FWD = 3 /* forward-only k_pass */,
       PROMP_KERNEL_EXCHANGE = 4 /* the ranks' exchange of [Theta+K+2] floats (all-reduce, or all-gather + ordered sum) */,
       PROMP_KERNEL_SCATTER = 5 /* k_scatter_partition's launches that deal a step's paths to its minibatches' slabs
                                   (promp_optimize_minibatch); the same kernel filling a selection's slab is not counted */,
       PROMP_KERNEL_COUNT = 6 };
int promp_prof_enable(promp_ctx* ctx, int on);
int promp_prof_read(promp_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches, int64_t* rows);
/* The fused pass kernels run their float32-equivalent products as a two-term FP16 split (promp_amd/csrc/promp_device.h); FP16 has a
 * range, so cotangents carry per-wave powers of two that follow the data.  out2 receives, and the call clears, how many segments
 * (a workgroup's share of a task's rows) were walked a second time since the last call because a cotangent left the format at the
 * scale its wave had chosen: k_pass [0], k_chain_hvp [1].  Diagnostics only -- heavy-tailed importance ratios (a policy far from the
 * one that sampled) cost time, never accuracy; the reference has no counterpart. */
int promp_split_events(promp_ctx* ctx, int64_t* out2);
int promp_device_info(promp_ctx* ctx, char* name_out, size_t name_bytes, int32_t* n_cus, int32_t* clock_mhz);

#ifdef __cplusplus
}
#endif
#endif /* PROMP_HIP_H */
