// promp_kernels_policy.h -- task-level reductions, Adam and the rollout-time forward pass (reference rows a10-a14).
//
//   k_reduce_task  : fixed-order sum of a task's per-workgroup partials + the update that consumes it, in a launch of its own
//                    behind the pass (every pass family's default since it was measured; k_chain_hvp's reduction inside the
//                    pass launch stays available: promp_set_schedule)
//   The final stage of an evaluation, each piece stated once: final_column_sum (one column of red, by task quarters),
//   final_stats_row (the statistics from the K + 2 scalar sums), theta_entry_step / alpha_entry_step (one entry's step under a
//   rule type of promp_kernels_step_sizes.h), and three bodies over them:
//   k_reduce_final : task sum of the per-task gradients and scalars                          (K14)
//   k_mean_adam    : mean over the global meta-batch + tf.train.AdamOptimizer step            (K14)
//   k_final_adam   : the two above in one launch (single rank)
//   k_mean_outer / k_final_outer : the mean and the fused body's general instances -- any rule and arguments of
//                    promp_set_outer_optimizer, and in k_mean_outer the clip by the global norm; launched only when the settings
//                    are not the default ones (final_stage_plan, promp_plan.h, which also decides every grid)
//                    (the *_ss instances carry Theta more columns: trainable step sizes, promp_kernels_step_sizes.h;
//                    the plain ones are the launches and arguments of a library without the feature)
//   k_policy_forward : mean network under each task's current parameters (get_actions)
#pragma once
#include "promp_device.h"
#include "promp_kernels_chain.h"
#include "promp_kernels_pass.h"
#include "promp_kernels_step_sizes.h"

// ---------------------------------------------------------------------------------------------
// Reductions over the per-workgroup partials of each task (fixed order => reproducible).
// grid = (ceil((NP+EXTRA)/256), n_tasks)
// ---------------------------------------------------------------------------------------------
struct ReduceArgs {
    const float* partials;
    int partial_stride;
    const int* task_wg_offsets;  // [tasks+1]: workgroups of task i are [o[i], o[i+1])
    int NP;                      // Theta
    const float* step_sizes;     // [Theta]
    // mode 0 (inner step): next[i] = cur[i] - alpha * g ; scal[i] = {loss, kl}
    // mode 1 (outer)     : lam[i] = g ; v[i] = alpha * g ; scal[i] = {loss, kl}
    // mode 2 (hvp)       : lam[i] += g ; v[i] = alpha * lam[i] ; scal[i] = {-, kl}
    // mode 3 (plain)     : lam[i] = g ; scal
    // mode 4 (scalars)   : scal only (forward-only passes write no gradient)
    int mode;
    const float* cur;            // [Theta] or [tasks][Theta]
    long long cur_task_stride;
    float* next;                 // [tasks][Theta]
    float* lam;                  // [tasks][Theta]
    float* v;                    // [tasks][Theta]
    float* scal;                 // [tasks][2]
    // mode 0 only, optional: the same step / scalars a second time (promp_inner_adapt leaves its result where the first
    // epoch of the following optimisation would have computed it: its adaptation chain and inner scalars)
    float* next2;
    float* scal2;
};

// KEEP_G (k_reduce_task_keep, mode 0): the summed gradient itself goes to ginner [tasks][Theta] as well (trainable step sizes,
// promp_kernels_step_sizes.h: the backward sweep multiplies it with the multiplier of the step behind it).  k_reduce_task is
// the instance without, with the arguments it always had.
template <bool KEEP_G>
PROMP_DEV void reduce_task_body(const ReduceArgs& a, float* ginner) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int task = blockIdx.y;
    if (j >= a.NP + 2) return;
    if (a.mode == 4 && j < a.NP) return;
    float g = 0.f;
    const int wg0 = a.task_wg_offsets[task], wg1 = a.task_wg_offsets[task + 1];
    // eight rows per round, all requested together (the rows sit in other CUs' cache lines or in memory: the kernel is one
    // or two memory round trips long, so what matters is how many loads are in flight); rows past the task's last are
    // clamped to a valid row and masked by a multiplication, which keeps the loads unconditional.  Added in slot order.
    for (int wb = wg0; wb < wg1; wb += 8) {
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int wg = wb + q < wg1 ? wb + q : wg1 - 1;
            x[q] = a.partials[(long long)wg * a.partial_stride + j] * (wb + q < wg1 ? 1.f : 0.f);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) g += x[q];
    }
    if (j >= a.NP) {
        a.scal[task * 2 + (j - a.NP)] = g;
        if (a.scal2 != nullptr) a.scal2[task * 2 + (j - a.NP)] = g;
        return;
    }
    const long long tj = (long long)task * a.NP + j;
    if (a.mode == 0) {
        const float nx = a.cur[(long long)task * a.cur_task_stride + j] - a.step_sizes[j] * g;
        a.next[tj] = nx;
        if (a.next2 != nullptr) a.next2[tj] = nx;
        if (KEEP_G) ginner[tj] = g;
        return;
    }
    float lam = g;
    if (a.mode == 2) lam += a.lam[tj];
    a.lam[tj] = lam;
    if (a.mode == 3) return;
    a.v[tj] = a.step_sizes[j] * lam;
}
__global__ void __launch_bounds__(256) k_reduce_task(ReduceArgs a) { reduce_task_body<false>(a, nullptr); }
__global__ void __launch_bounds__(256) k_reduce_task_keep(ReduceArgs a, float* ginner) { reduce_task_body<true>(a, ginner); }

// Task sum of lam (gradient) and of the per-task scalars -> red[NP + K + 2]
//   red[0..NP)      = sum_i lam[i][j]
//   red[NP]         = sum_i J_i                     (outer surrogate)
//   red[NP+1+k]     = sum_i KL^k_i
//   red[NP+1+K]     = sum_i outer KL_i
//   red[NP+K+2+j]   = sum_i galpha[i][j]            (trainable step sizes only: Theta more columns behind the others)
struct FinalArgs {
    const float* lam;
    int NP, K, n_tasks;
    const float* scal_inner;  // [K][tasks][2]
    const float* scal_outer;  // [tasks][2]
    float* red;
    int want_grad;
};
// trainable step sizes: what the *_ss instances of the final stage take beside the arguments above
struct StepSizeArgs {
    const float* galpha;      // [tasks][NP] per-task step-size gradients (k_step_size_grad)
    float* alpha;             // the step sizes and their Adam slots: the same Adam step as theta's (lr_t, do_update, n_trainable)
    float* alpha_m;
    float* alpha_v;
    float* alpha_grad_mean;   // [NP] task-mean step-size gradient (promp_get_step_size_grad)
};

// One task quarter of a [tasks][NP] column: thread (c, q) adds the tasks i = q, q + 4, ... of column j
// (up to 12 tasks of the quarter requested together, clamped + masked like k_reduce_task; order i = q, q + 4, ...)
PROMP_DEV float final_quarter_sum(const float* rows, int NP, int n_tasks, int j, int q) {
    float s = 0.f;
    for (int ib = q; ib < n_tasks; ib += 48) {
        float x[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            const int i = ib + 4 * u;
            x[u] = rows[(long long)(i < n_tasks ? i : q) * NP + j] * (i < n_tasks ? 1.f : 0.f);
        }
#pragma unroll
        for (int u = 0; u < 12; ++u) s += x[u];
    }
    return s;
}

// The column sum: task quarter q of column j of red's layout above (0 past jend, the launch's last column + 1).
template <bool SS>
PROMP_DEV float final_column_sum(const FinalArgs& a, const float* galpha, int j, int q, int jend) {
    float s = 0.f;
    if (j < a.NP) {
        if (a.want_grad) s = final_quarter_sum(a.lam, a.NP, a.n_tasks, j, q);
    } else if (j == a.NP) {
        for (int i = q; i < a.n_tasks; i += 4) s += a.scal_outer[i * 2 + 0];
    } else if (j <= a.NP + a.K) {
        const int k = j - a.NP - 1;
        for (int i = q; i < a.n_tasks; i += 4) s += a.scal_inner[((long long)k * a.n_tasks + i) * 2 + 1];
    } else if (j == a.NP + a.K + 1) {
        for (int i = q; i < a.n_tasks; i += 4) s += a.scal_outer[i * 2 + 1];
    } else if (SS && j < jend) {
        s = final_quarter_sum(galpha, a.NP, a.n_tasks, j - (a.NP + a.K + 2), q);
    }
    return s;
}
// the four quarter sums of column c, added in a fixed order
PROMP_DEV float final_column_total(const float (*part)[64], int c) { return (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]); }

// grid = final_stage_launch's reduce_grid (promp_plan.h): ceil((NP + K + 2) / 64) -- k_reduce_final_ss: ceil((2 NP + K + 2) / 64) --,
// block = 256: 64 columns x 4 task quarters.  Thread (c, q) adds the tasks i = q, q+4, ... of column c (10 dependent-latency
// steps instead of 40 at M = 40).
template <bool SS>
PROMP_DEV void reduce_final_body(const FinalArgs& a, const float* galpha, float (*part)[64]) {
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    const int jend = a.NP + a.K + 2 + (SS ? a.NP : 0);
    part[q][c] = final_column_sum<SS>(a, galpha, j, q, jend);
    __syncthreads();
    if (q == 0 && j < jend) a.red[j] = final_column_total(part, c);
}
__global__ void __launch_bounds__(256) k_reduce_final(FinalArgs a) {
    __shared__ float part[4][64];
    reduce_final_body<false>(a, nullptr, part);
}
__global__ void __launch_bounds__(256) k_reduce_final_ss(FinalArgs a, const float* galpha) {
    __shared__ float part[4][64];
    reduce_final_body<true>(a, galpha, part);
}

// Mean over the global meta-batch + Adam.  red holds SUMS over all tasks (after the all-reduce).
// stats[0] = loss = mean_i J_i + mean_k(eta_k * mean_i KL^k_i); stats[1+k] = inner_kl[k]; stats[1+K] = outer_kl
struct AdamArgs {
    float* theta;
    float* m;
    float* v;
    const float* red;
    float* grad_mean;  // [NP] task-mean gradient (kept for promp_meta_grad's output)
    float* stats;      // [K+2]
    float eta[PROMP_ETA_MAX];   // inner KL coefficients, by value (K <= PROMP_ETA_MAX): no host -> device copy per optimisation
    int NP, K, A;
    float inv_tasks;
    float lr_t;        // lr * sqrt(1-b2^t)/(1-b1^t); 0 => no parameter update (stats / grad only)
    int do_update;
    int n_trainable;   // parameters [n_trainable, NP) are left alone (learn_std = False: the trailing log_std entries)
    // promp_optimize_begin's last launch: both statistics slots go straight to page-locked host memory, followed by a
    // sequence number the host polls (no copy operation, no event on the queue)
    float* host_stats;       // [2 (K + 2) + 1] or NULL; the last entry: the smallest log_std entry of theta as it is now
    unsigned* host_seq;
    unsigned seq;
};
// (called by the one thread that has just written stats[0 .. K+2); the second slot was written by an earlier launch)
PROMP_DEV void publish_stats(const AdamArgs& a) {
    if (a.host_stats == nullptr) return;
    for (int i = 0; i < 2 * (a.K + 2); ++i) a.host_stats[i] = a.stats[i];
    {   // (the publishing launch does not update theta: what is read here is what the next inner step will see)
        float lo = a.theta[a.NP - a.A];
        for (int i = 1; i < a.A; ++i) lo = fminf(lo, a.theta[a.NP - a.A + i]);
        a.host_stats[2 * (a.K + 2)] = lo;
    }
    release_store_system(a.host_seq, a.seq);
}

// The statistics row, by one thread: sums[0] = sum_i J_i, sums[1..K] = sum_i KL^k_i, sums[K + 1] = sum_i outer KL_i
PROMP_DEV void final_stats_row(const AdamArgs& a, const float* sums) {
    float pen = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const float ikl = sums[1 + k] * a.inv_tasks;
        a.stats[1 + k] = ikl;
        pen += a.eta[k] * ikl;
    }
    a.stats[0] = sums[0] * a.inv_tasks + pen / (float)a.K;
    a.stats[1 + a.K] = sums[1 + a.K] * a.inv_tasks;
    publish_stats(a);
}
// One entry of theta: the task-mean gradient g (kept unclipped) and the rule's step (R: promp_kernels_step_sizes.h)
template <class R>
PROMP_DEV void theta_entry_step(const R& r, const AdamArgs& a, int j, float g) {
    a.grad_mean[j] = g;
    if (a.do_update && j < a.n_trainable) r.step(a.theta, a.m, a.v, j, r.clipped(g), a.lr_t);
}
// and of alpha, from the sum t of its column
template <class R>
PROMP_DEV void alpha_entry_step(const R& r, const AdamArgs& a, const StepSizeArgs& ss, int ja, float t) {
    step_size_entry_step(r, ss.alpha, ss.alpha_m, ss.alpha_v, ss.alpha_grad_mean, ja, t * a.inv_tasks, a.do_update && ja < a.n_trainable,
                         ja < a.n_trainable, a.lr_t);
}

// Mean + step.  grid = final_stage_launch's mean_grid: ceil((NP + 1) / 256) -- SS (the *_ss instances): ceil((2 NP + 1) / 256), the
// step sizes' step from red[NP + K + 2 + j] behind theta's --, block = 256
template <bool SS, class R>
PROMP_DEV void mean_step_body(const AdamArgs& a, const StepSizeArgs& ss, const R& r) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < a.NP) {
        theta_entry_step(r, a, j, a.red[j] * a.inv_tasks);
    } else if (j == a.NP) {
        final_stats_row(a, a.red + a.NP);
    } else if (SS && j <= 2 * a.NP) {
        const int ja = j - a.NP - 1;
        alpha_entry_step(r, a, ss, ja, a.red[a.NP + a.K + 2 + ja]);
    }
}
__global__ void __launch_bounds__(256) k_mean_adam(AdamArgs a) { mean_step_body<false>(a, StepSizeArgs{}, PlainAdamRule{}); }
__global__ void __launch_bounds__(256) k_mean_adam_ss(AdamArgs a, StepSizeArgs ss) { mean_step_body<true>(a, ss, PlainAdamRule{}); }

// Fixed-order exchange: the ranks' vectors side by side ([nranks][n], ncclAllGather) added in rank order -- the same additions in
// the same order on every rank.
__global__ void __launch_bounds__(256) k_sum_ranks(const float* gathered, float* out, int n, int nranks) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float s = gathered[j];
    for (int r = 1; r < nranks; ++r) s += gathered[(long long)r * n + j];
    out[j] = s;
}

// Sum + step in one launch, for the single-rank case (no all-reduce in between): k_reduce_final + the mean kernel.  Column sums
// in the same order as k_reduce_final (bitwise the same red[]); the thread that finishes a parameter column steps its entry (so
// no clip: the other columns' sums do not exist yet); one extra workgroup re-sums the K + 2 scalar columns and writes the statistics.
// grid = final_stage_launch's fused_grid: the reduce grid + 1, block = 256
template <bool SS, class R>
PROMP_DEV void final_step_body(const FinalArgs& a, const AdamArgs& ad, const StepSizeArgs& ss, const R& r, float (*part)[64], float* sums) {
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const bool stats_block = blockIdx.x == gridDim.x - 1;
    const int j = stats_block ? a.NP + c : blockIdx.x * 64 + c;
    const int jend = a.NP + a.K + 2 + (SS && !stats_block ? a.NP : 0);
    part[q][c] = final_column_sum<SS>(a, ss.galpha, j, q, jend);
    __syncthreads();
    if (q == 0 && j < jend) {
        const float t = final_column_total(part, c);
        if (!stats_block) a.red[j] = t;
        sums[c] = t;
        if (!stats_block && j < a.NP) theta_entry_step(r, ad, j, t * ad.inv_tasks);
        else if (SS && !stats_block && j >= a.NP + a.K + 2) alpha_entry_step(r, ad, ss, j - (a.NP + a.K + 2), t);
    }
    if (!stats_block) return;
    __syncthreads();
    if (threadIdx.x == 0) final_stats_row(ad, sums);
}
__global__ void __launch_bounds__(256) k_final_adam(FinalArgs a, AdamArgs ad) {
    __shared__ float part[4][64];
    __shared__ float sums[64];
    final_step_body<false>(a, ad, StepSizeArgs{}, PlainAdamRule{}, part, sums);
}
__global__ void __launch_bounds__(256) k_final_adam_ss(FinalArgs a, AdamArgs ad, StepSizeArgs ss) {
    __shared__ float part[4][64];
    __shared__ float sums[64];
    final_step_body<true>(a, ad, ss, PlainAdamRule{}, part, sums);
}

// ---------------------------------------------------------------------------------------------
// The general final stage (promp_set_outer_optimizer): the bodies above over GeneralRule, with the rule, its arguments and the
// clip as launch arguments.  The plain instances carry none of them -- a run-time branch in them is paid by every default step
// (profiles/step_size_timing.txt) --, and final_stage_plan launches these only for settings that are not the default ones.
// ---------------------------------------------------------------------------------------------
// Sum of squares of the task-mean gradient over the trained entries -- theta's [0, n_trainable) and, SS, alpha's --, by EVERY
// workgroup of k_mean_outer for itself: red is Theta or 2 Theta floats (24 KB at 5 900 parameters) that sit in L2 behind
// k_reduce_final or the exchange, so no workgroup waits for another and no launch is added.  float64, one fixed order: thread t
// adds the entries t, t + 256, ... (theta's, then alpha's), then a binary tree over the 256 partial sums in LDS -- the same bits
// in every workgroup.  buf: 256 doubles.
// (eight entries of a thread requested together, clamped + selected like final_quarter_sum's rows: at 32 k parameters a thread has
// 125 entries, and one L2 round trip per entry would cost more than the launch)
PROMP_DEV double outer_sq_sum(const float* x, int n, float inv, double s) {
    const int t = threadIdx.x;
    for (int jb = t; jb < n; jb += 8 * 256) {
        float g[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = jb + 256 * u;
            const float v = x[j < n ? j : jb];
            g[u] = j < n ? v * inv : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)g[u] * (double)g[u];
    }
    return s;
}
template <bool SS>
PROMP_DEV double outer_sq_norm(const AdamArgs& a, double* buf) {
    const int t = threadIdx.x;
    double s = outer_sq_sum(a.red, a.n_trainable, a.inv_tasks, 0.0);
    if (SS) s = outer_sq_sum(a.red + a.NP + a.K + 2, a.n_trainable, a.inv_tasks, s);
    buf[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) buf[t] += buf[t + w];
        __syncthreads();
    }
    return buf[0];
}

// The clip's factor, by every thread of k_mean_outer: scale = n > c ? c / n : 1 is exactly 1 when the clip is off or not active
// (tf.clip_by_global_norm computes c * min(1 / n, 1 / c): the same up to the last bit); a non-finite norm makes every update
// non-finite, as there.  One thread leaves n for promp_get_grad_norm.
template <bool SS>
PROMP_DEV float outer_clip_scale(const AdamArgs& a, const OuterOptArgs& o, float* norm_out, double* buf) {
    float scale = 1.f;
    if (o.max_norm > 0.f) {       // (uniform over the grid: every thread reaches the barriers inside)
        const float n = (float)sqrt(outer_sq_norm<SS>(a, buf));
        scale = n > o.max_norm ? o.max_norm / n : 1.f;
        if (!(fabsf(n) <= 3.402823466e38f)) scale = n - n;       // inf or NaN: NaN
        if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = n;
    }
    return scale;
}
// mean + step under any rule, with the clip; sum + step under any rule (no clip: see final_step_body).
// Grids and blocks as the plain instances'.
__global__ void __launch_bounds__(256) k_mean_outer(AdamArgs a, OuterOptArgs o, float* norm_out) {
    __shared__ double buf[256];
    mean_step_body<false>(a, StepSizeArgs{}, GeneralRule{o, outer_clip_scale<false>(a, o, norm_out, buf)});
}
__global__ void __launch_bounds__(256) k_mean_outer_ss(AdamArgs a, StepSizeArgs ss, OuterOptArgs o, float* norm_out) {
    __shared__ double buf[256];
    mean_step_body<true>(a, ss, GeneralRule{o, outer_clip_scale<true>(a, o, norm_out, buf)});
}
__global__ void __launch_bounds__(256) k_final_outer(FinalArgs a, AdamArgs ad, OuterOptArgs o) {
    __shared__ float part[4][64];
    __shared__ float sums[64];
    final_step_body<false>(a, ad, StepSizeArgs{}, GeneralRule{o, 1.f}, part, sums);
}
__global__ void __launch_bounds__(256) k_final_outer_ss(FinalArgs a, AdamArgs ad, StepSizeArgs ss, OuterOptArgs o) {
    __shared__ float part[4][64];
    __shared__ float sums[64];
    final_step_body<true>(a, ad, ss, GeneralRule{o, 1.f}, part, sums);
}

// dst[i][:] = src[:] for i < n_tasks   (MetaPolicy.switch_to_pre_update)
__global__ void __launch_bounds__(256) k_replicate(float* dst, const float* src, int NP, int n_tasks) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < NP)
        for (int i = 0; i < n_tasks; ++i) dst[(long long)i * NP + j] = src[j];
}

// Elementwise glue of promp_constraint_hvp (products with the adaptation Jacobian J = I - diag(alpha) H):
//   mode 0:  dir += alpha * lam                       (dir <- J dir, lam = -H dir from the pass before)
//   mode 1:  w = -lam ;      dir = alpha * w          (w <- H_KL u, lam = -H_KL u)
//   mode 2:  w += lam ;      dir = alpha * w          (w <- J^T w, lam = -H (alpha * w))
// grid = (ceil(NP / 256), tasks)
__global__ void __launch_bounds__(256) k_jstep(float* dir, float* w, const float* lam, const float* alpha, int NP, int mode) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= NP) return;
    const long long tj = (long long)blockIdx.y * NP + j;
    if (mode == 0) {
        dir[tj] += alpha[j] * lam[tj];
        return;
    }
    const float x = (mode == 1) ? -lam[tj] : w[tj] + lam[tj];
    w[tj] = x;
    dir[tj] = alpha[j] * x;
}

// ---------------------------------------------------------------------------------------------
// k_policy_forward: mean network of every task's CURRENT parameters on a small batch of observations
// (MetaGaussianMLPPolicy.get_actions, policies/meta_gaussian_mlp_policy.py:99-157: [tasks][B][O] -> [tasks][B][A]).
// Rollout-time inference is a few hundred rows per environment step: one workgroup per task, one thread per row,
// weights read through the scalar/L1 path; it is latency-, not throughput-bound.
// grid = tasks, block = 256
// ---------------------------------------------------------------------------------------------
struct ForwardArgs {
    const float* obs;          // [tasks][B][O]
    const float* theta_tasks;  // [tasks][Theta]
    float* mean;               // [tasks][B][A]
    int B, O, A, H1, H2;
};

__global__ void __launch_bounds__(256) k_policy_forward(ForwardArgs a) {
    const int task = blockIdx.x;
    const int O = a.O, A = a.A, H1 = a.H1, H2 = a.H2;
    const Mlp2Layout lay = mlp2_layout(O, H1, H2, A);
    const float* th = a.theta_tasks + (long long)task * lay.NP;
    for (int row = threadIdx.x; row < a.B; row += 256) {
        const float* x = a.obs + ((long long)task * a.B + row) * O;
        float h1[128], h2[128];   // hidden sizes up to 128
        for (int j = 0; j < H1; ++j) {
            float z = th[lay.b1 + j];
            for (int k = 0; k < O; ++k) z = fmaf(x[k], th[k * H1 + j], z);
            h1[j] = fast_tanh(z);
        }
        for (int j = 0; j < H2; ++j) {
            float z = th[lay.b2 + j];
            for (int k = 0; k < H1; ++k) z = fmaf(h1[k], th[lay.W2 + k * H2 + j], z);
            h2[j] = fast_tanh(z);
        }
        for (int j = 0; j < A; ++j) {
            float z = th[lay.b3 + j];
            for (int k = 0; k < H2; ++k) z = fmaf(h2[k], th[lay.W3 + k * A + j], z);
            a.mean[((long long)task * a.B + row) * A + j] = z;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Conjugate gradients on the device (promp_cg_solve): the vector side of ConjugateGradientOptimizer's solve
// (optimizers/conjugate_gradient_optimizer.py:325-354, conjugate_gradients) between two products, in ONE launch of one workgroup -- the vectors are
// Theta floats (6 k ... 70 k), the launch is a link in a chain of dependent launches and costs what any of them costs.
// Sums in a fixed order (thread-strided, then a tree over the workgroup) in float64; the vectors stay float32 like the
// NumPy arrays of the host form.
// ---------------------------------------------------------------------------------------------
// theta = theta0 + s x  (FiniteDifferenceHvp: the parameters the displaced constraint gradient is taken at; one rounding)
__global__ void __launch_bounds__(256) k_cg_displace(float* theta, const float* theta0, const float* x, float s, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) theta[j] = __builtin_fmaf(s, x[j], theta0[j]);
}

struct CgArgs {
    const float* g_ahead;    // finite differences: the constraint gradient at theta0 + eps v; exact: the task sums of the product
    const float* g_behind;   // ... at theta0 - eps v (symmetric) / at theta0 (one-sided); NULL: nothing is subtracted
    float div_h, mul_s;      // H v = ((g_ahead - g_behind) / div_h) * mul_s   (2 eps or eps, 1; exact: 1, 1 / tasks)
    float reg;               // + reg v
    float *x, *r, *d, *hd;   // solution, residual, search direction, (H + reg I) v
    double* scal;            // [0] r.r   [1] d.(H + reg I)d of the last iteration   [2] != 0: converged   [3] x.(H + reg I)x
    float tol;               // residual_tol
    int n;
    int mode;                // 2: x = 0, d = r (= b), scal[0] = r.r;   0: one iteration along d;   1: the closing product on x
};
PROMP_DEV double cg_block_sum(double v, double* buf) {
    const int t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    return buf[0];
}
// grid = 1, block = 1024
__global__ void __launch_bounds__(1024) k_cg_step(CgArgs a) {
    __shared__ double buf[1024];
    const int t = threadIdx.x;
    if (a.mode == 2) {
        double s = 0.0;
        for (int j = t; j < a.n; j += 1024) {
            const float b = a.r[j];
            a.x[j] = 0.f;
            a.d[j] = b;
            s += (double)b * (double)b;
        }
        s = cg_block_sum(s, buf);
        if (t == 0) {
            a.scal[0] = s; a.scal[1] = 0.0; a.scal[2] = 0.0; a.scal[3] = 0.0;
        }
        return;
    }
    const float* v = a.mode == 1 ? a.x : a.d;
    double dot = 0.0;
    for (int j = t; j < a.n; j += 1024) {
        const float gb = a.g_behind ? a.g_behind[j] : 0.f;
        const float h = __builtin_fmaf(a.reg, v[j], ((a.g_ahead[j] - gb) / a.div_h) * a.mul_s);
        a.hd[j] = h;
        dot += (double)v[j] * (double)h;
    }
    dot = cg_block_sum(dot, buf);
    if (a.mode == 1) {
        if (t == 0) a.scal[3] = dot;
        return;
    }
    const double res = a.scal[0];
    if (a.scal[2] != 0.0) return;          // converged in an earlier iteration: the host form has left its loop (uniform: no barrier is skipped by a part of the block)
    const float step = (float)(res / dot);
    double nres = 0.0;
    for (int j = t; j < a.n; j += 1024) {
        a.x[j] = __builtin_fmaf(step, a.d[j], a.x[j]);
        const float rr = __builtin_fmaf(-step, a.hd[j], a.r[j]);
        a.r[j] = rr;
        nres += (double)rr * (double)rr;
    }
    nres = cg_block_sum(nres, buf);
    const float beta = (float)(nres / res);
    for (int j = t; j < a.n; j += 1024) a.d[j] = __builtin_fmaf(beta, a.d[j], a.r[j]);
    if (t == 0) {
        a.scal[0] = nres;
        a.scal[1] = dot;
        if (nres < (double)a.tol) a.scal[2] = 1.0;
    }
}
