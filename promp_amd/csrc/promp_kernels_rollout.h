// promp_kernels_rollout.h -- rollout-side kernels.
//
//   k_policy_step   : one environment step of EVERY environment of the meta-batch: mean network under each task's current
//                     parameters, Gaussian exploration noise drawn on the device (Philox4x32-10 + Box-Muller), action =
//                     mean + exp(log_std) * noise; observation, action and mean are written straight into the sampling
//                     step's slab at row (task, env, t) and only the actions go back to the host
//                     (policies/meta_gaussian_mlp_policy.py:99-157 + samplers/meta_sampler.py:87-125 of the reference:
//                     one sess.run plus a Python loop per environment step).
//   k_point_rollout : a whole fixed-horizon rollout of the 2-D point-mass meta-environment of BASELINE config 1
//                     (run_scripts/pro-mp_run_point_mass.py: normalize(MetaPointEnvCorner())), one thread per environment:
//                       envs/point_envs/point_env_2d_corner.py:37   state += clip(action, -0.2, 0.2)
//                       envs/point_envs/point_env_2d_corner.py:62-81 reward: dense -|s' - g|, dense_squared -|s' - g|^2,
//                                                                     sparse (progress towards the goal once the point has
//                                                                     left the start region and the goal is the nearest corner)
//                       envs/normalized_env.py:109-123              the wrapper maps policy actions in [-10, 10] onto the
//                                                                     environment's action box [-0.2, 0.2] and clips
//                     no early termination (point_env_2d_corner.py:39).  The exploration noise is either given by the caller
//                     (reproducible from a host RNG; the parity tests compare with the reference environment step by step)
//                     or drawn on the device.
//   k_point_family_rollout : the same launch for the reference's three fixed-horizon point-mass meta-environments (corner, walls,
//                     momentum; envs/point_envs/point_env_2d_walls.py, point_env_2d_momentum.py), at the end of this file.
#pragma once
#include "promp_device.h"

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter-based, so every
// (environment, time step) draws its numbers independently of launch geometry.  oracle/philox.py restates it and is
// pinned by the published known-answer vectors.
struct Philox4 {
    unsigned x, y, z, w;
};
PROMP_HD Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 r;
    r.x = c0; r.y = c1; r.z = c2; r.w = c3;
    return r;
}
// two standard normals from two 32-bit words (Box-Muller; u1 in (0, 1], u2 in [0, 1))
PROMP_HD void box_muller(unsigned a, unsigned b, float& n0, float& n1) {
    const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    const float ang = 6.283185307179586f * u2;
    n0 = r * cosf(ang);
    n1 = r * sinf(ang);
}
// action-noise of row `row`, action pair `pair` (actions 2 pair, 2 pair + 1), stream `stream` (sampling step)
PROMP_HD void action_noise(unsigned long long seed, unsigned long long row, unsigned pair, unsigned stream, float& n0, float& n1) {
    const Philox4 r = philox4x32_10((unsigned)row, (unsigned)(row >> 32), pair, stream, (unsigned)seed, (unsigned)(seed >> 32));
    box_muller(r.x, r.y, n0, n1);
}

// ---- start states drawn on the device: the reset() of the point-mass classes (point_env_2d_corner.py:50, point_env_2d_walls.py:60,
// point_env_2d_momentum.py:51-52, point_env_2d.py:37, point_env_2d_v2.py:40 of the reference: np.random.uniform over a box, or zeros).
// Coordinates 2 p and 2 p + 1 of the reset() filed under start-table row `row` come from ONE Philox block:
//   counter (lo32(row), hi32(row), 0x80000000 | p, stream), key (lo32(seed), hi32(seed))
// row = s * n_envs + env, s the row of the host's start table (0: the initial states; s + 1: the state an environment continues from
// after an episode that ends at step s); the fixed-horizon rollouts have row = env.  The high bit of word 2 keeps these blocks apart
// from the action-noise blocks of the same (seed, stream), whose word 2 is an action pair below 32.  Words (x, y) give coordinate
// 2 p, (z, w) coordinate 2 p + 1: u = ((a >> 5) 2^26 + (b >> 6)) / 2^53, a float64 in [0, 1) (53 bits, every step exact), and
// value = lo + (hi - lo) u with every operation rounded on its own, so that NumPy restates it bit for bit; lo == hi yields lo.
struct PointStartBox {
    double lo[4], hi[4];       // coordinate k < state_dim of every reset()
    unsigned long long seed;   // the key: its own, beside the action noise's
};
PROMP_HD double start_uniform(unsigned a, unsigned b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}
PROMP_HD double start_value(double lo, double hi, double u) {
#pragma clang fp contract(off)
    const double width = hi - lo;
    const double part = width * u;
    return lo + part;
}
// the first O (2 or 4) coordinates of the reset() under `row`
PROMP_HD void point_start_state(const PointStartBox& bx, unsigned stream, unsigned long long row, int O, double* s) {
    for (int p = 0; 2 * p < O; ++p) {
        const Philox4 r = philox4x32_10((unsigned)row, (unsigned)(row >> 32), 0x80000000u | (unsigned)p, stream, (unsigned)bx.seed,
                                        (unsigned)(bx.seed >> 32));
        s[2 * p] = start_value(bx.lo[2 * p], bx.hi[2 * p], start_uniform(r.x, r.y));
        s[2 * p + 1] = start_value(bx.lo[2 * p + 1], bx.hi[2 * p + 1], start_uniform(r.z, r.w));
    }
}
// the table a host would have uploaded: out [n_rows][n_envs][state_dim].  grid = ceil(n / 256), block = 256: one thread per reset()
struct PointStartsArgs {
    PointStartBox bx;
    unsigned stream;
    int state_dim;
    long long n;               // n_rows * n_envs
    double* out;
};
__global__ void __launch_bounds__(256) k_point_starts(PointStartsArgs a) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.n) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    point_start_state(a.bx, a.stream, (unsigned long long)row, a.state_dim, s);
    for (int k = 0; k < a.state_dim; ++k) a.out[row * a.state_dim + k] = s[k];
}

// mean network of one observation row under flat parameters th (hidden widths <= 128, act_dim <= 8).  EXACT_TANH: tanhf instead of
// fast_tanh, whose absolute error of ~1e-7 per unit is what the momentum environment's double integrator sums up (see
// k_point_family_rollout)
template <bool EXACT_TANH>
PROMP_DEV void mlp_mean_t(const float* th, const float* x, int O, int A, int H1, int H2, float* mean) {
    const Mlp2Layout lay = mlp2_layout(O, H1, H2, A);
    float h1[128], h2[128];
    for (int j = 0; j < H1; ++j) {
        float z = th[lay.b1 + j];
        for (int k = 0; k < O; ++k) z = fmaf(x[k], th[k * H1 + j], z);
        h1[j] = EXACT_TANH ? tanhf(z) : fast_tanh(z);
    }
    for (int j = 0; j < H2; ++j) {
        float z = th[lay.b2 + j];
        for (int k = 0; k < H1; ++k) z = fmaf(h1[k], th[lay.W2 + k * H2 + j], z);
        h2[j] = EXACT_TANH ? tanhf(z) : fast_tanh(z);
    }
    for (int j = 0; j < A; ++j) {
        float z = th[lay.b3 + j];
        for (int k = 0; k < H2; ++k) z = fmaf(h2[k], th[lay.W3 + k * A + j], z);
        mean[j] = z;
    }
}
PROMP_DEV void mlp_mean(const float* th, const float* x, int O, int A, int H1, int H2, float* mean) {
    mlp_mean_t<false>(th, x, O, A, H1, H2, mean);
}

struct PolicyStepArgs {
    const float* obs_in;        // [tasks][B][O] observations of this environment step
    const float* theta_tasks;   // [tasks][Theta]
    float *obs, *act, *mean;    // where the rows go: row = env * row_env_stride + t * row_t_stride, env = task * B + b
    long long row_env_stride, row_t_stride;   // fixed-length rollout: (T, 1) into the slab; ragged collection: (1, tasks * B) into the staging rows
    float* old_ls;              // [tasks][A] log_std reported in agent_infos (written at t = 0)
    float* actions_out;         // [tasks][B][A]
    int B, T, t, O, A, H1, H2, NP;
    int clip_infos;             // pre-update policy: agent_infos carry max(log_std, log(min_std)); the noise scale never does
    float min_log_std;
    unsigned long long seed;
    unsigned stream;
};

// grid = (ceil(B / 64), tasks), block = 64: one thread per environment
__global__ void __launch_bounds__(64) k_policy_step(PolicyStepArgs a) {
    const int task = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
    const float* th = a.theta_tasks + (long long)task * a.NP;
    const int oS = a.NP - a.A;
    if (a.t == 0 && blockIdx.x == 0 && (int)threadIdx.x < a.A) {
        const float ls = th[oS + threadIdx.x];
        a.old_ls[task * a.A + threadIdx.x] = a.clip_infos ? fmaxf(ls, a.min_log_std) : ls;
    }
    if (b >= a.B) return;
    const long long env = (long long)task * a.B + b, row = env * a.row_env_stride + a.t * a.row_t_stride;
    const float* x = a.obs_in + env * a.O;
    float mean[8];
    mlp_mean(th, x, a.O, a.A, a.H1, a.H2, mean);
    for (int k = 0; k < a.O; ++k) a.obs[row * a.O + k] = x[k];
    for (int j = 0; j < a.A; j += 2) {
        float n0, n1;
        action_noise(a.seed, (unsigned long long)row, (unsigned)(j >> 1), a.stream, n0, n1);
        const float a0 = fmaf(expf(th[oS + j]), n0, mean[j]);
        a.mean[row * a.A + j] = mean[j];
        a.act[row * a.A + j] = a0;
        a.actions_out[env * a.A + j] = a0;
        if (j + 1 < a.A) {
            const float a1 = fmaf(expf(th[oS + j + 1]), n1, mean[j + 1]);
            a.mean[row * a.A + j + 1] = mean[j + 1];
            a.act[row * a.A + j + 1] = a1;
            a.actions_out[env * a.A + j + 1] = a1;
        }
    }
}

// Ragged collection (samplers/meta_sampler.py:100-125: an environment that reports `done` starts its next episode at once):
// promp_policy_step files the rows of vectorised step s under (s, env) in a staging area; when the host knows the episodes, the
// finished ones are copied into the step's slab in path order: path p = staging rows (start[p] + t, env[p]), t < len[p].
struct GatherPathsArgs {
    const float *obs_in, *act_in, *mean_in;   // staging rows [steps][n_envs]
    float *obs, *act, *mean;                  // the slab
    const int *path_env, *path_start, *path_row_offsets;
    int n_envs, O, A;
    const float* rew_in = nullptr;            // staged rewards [steps][n_envs], or NULL: the caller uploads the slab's rewards itself
    float* rew = nullptr;                     // the slab's rewards (read only with rew_in)
};
// grid = paths, block = 256
__global__ void __launch_bounds__(256) k_gather_paths(GatherPathsArgs a) {
    const int p = blockIdx.x, env = a.path_env[p], s0 = a.path_start[p], r0 = a.path_row_offsets[p], n = a.path_row_offsets[p + 1] - r0;
    const int W = a.O + 2 * a.A;
    for (int e = threadIdx.x; e < n * W; e += 256) {
        const int t = e / W, k = e - t * W;
        const long long src = (long long)(s0 + t) * a.n_envs + env, dst = r0 + t;
        if (k < a.O) a.obs[dst * a.O + k] = a.obs_in[src * a.O + k];
        else if (k < a.O + a.A) a.act[dst * a.A + (k - a.O)] = a.act_in[src * a.A + (k - a.O)];
        else a.mean[dst * a.A + (k - a.O - a.A)] = a.mean_in[src * a.A + (k - a.O - a.A)];
    }
    if (a.rew_in != nullptr)
        for (int t = threadIdx.x; t < n; t += 256) a.rew[r0 + t] = a.rew_in[(long long)(s0 + t) * a.n_envs + env];
}

// Some or all of a step's paths copied into B compact slabs in ONE launch -- the slabs of its minibatches (promp_optimize_minibatch;
// build_partition, promp_plan.h), or the one slab of its selection (promp_set_step_selection; selection_copy_table): source path p
// goes to slab copy[2p], rows [copy[2p + 1] + shift[slab], ...) of the pooled slabs -- everything a policy pass reads of a row --,
// or nowhere if copy[2p] < 0.  The walk over the observations also leaves, per (slab, task), the bits of the largest |observation|
// that k_obs_range would find on that compact slab (promp_kernels_pass.h; a maximum of bit patterns does not depend on the order
// it is taken in): one atomic per wave, into a table zeroed in front of the launch.
struct ScatterPartitionArgs {
    const float *obs_in, *act_in, *adv_in, *mean_in, *ls_in;   // the step's slabs (ls_in: NULL when log_std is one row per task)
    float *obs, *act, *adv, *mean, *ls;                         // the pooled slabs
    const int *src_row_offsets, *path_task;                     // the step's [paths + 1] / [paths]
    const int *copy, *shift;                                    // [paths][2] / [slabs]: rows between a slab's place and its offset
    unsigned* absmax;                                           // [slabs][tasks]
    int O, A, n_tasks;
};
// n consecutive floats: consecutive lanes on consecutive addresses, four loads in flight per lane
PROMP_DEV void scatter_span(float* dst, const float* src, long long n, int tid) {
    long long i = tid;
    for (; i + 768 < n; i += 1024) {
        const float v0 = src[i], v1 = src[i + 256], v2 = src[i + 512], v3 = src[i + 768];
        dst[i] = v0; dst[i + 256] = v1; dst[i + 512] = v2; dst[i + 768] = v3;
    }
    for (; i < n; i += 256) dst[i] = src[i];
}
// grid = the step's paths, block = 256
__global__ void __launch_bounds__(256) k_scatter_partition(ScatterPartitionArgs a) {
    const int p = blockIdx.x, tid = threadIdx.x, mb = a.copy[2 * p];
    if (mb < 0) return;
    const long long s0 = a.src_row_offsets[p], n = a.src_row_offsets[p + 1] - s0, r0 = (long long)a.copy[2 * p + 1] + a.shift[mb];
    {
        const float* src = a.obs_in + s0 * a.O;
        float* dst = a.obs + r0 * a.O;
        const long long nf = n * a.O;
        unsigned m = 0;
        long long i = tid;
        for (; i + 768 < nf; i += 1024) {
            const float v0 = src[i], v1 = src[i + 256], v2 = src[i + 512], v3 = src[i + 768];
            dst[i] = v0; dst[i + 256] = v1; dst[i + 512] = v2; dst[i + 768] = v3;
            const unsigned u0 = __builtin_bit_cast(unsigned, v0) & 0x7FFFFFFFu, u1 = __builtin_bit_cast(unsigned, v1) & 0x7FFFFFFFu;
            const unsigned u2 = __builtin_bit_cast(unsigned, v2) & 0x7FFFFFFFu, u3 = __builtin_bit_cast(unsigned, v3) & 0x7FFFFFFFu;
            const unsigned x = u0 > u1 ? u0 : u1, y = u2 > u3 ? u2 : u3, z = x > y ? x : y;
            m = z > m ? z : m;
        }
        for (; i < nf; i += 256) {
            const float v = src[i];
            dst[i] = v;
            const unsigned u = __builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu;
            m = u > m ? u : m;
        }
        float mf = __builtin_bit_cast(float, m);      // (compared as integers: the bit patterns of non-negative floats are ordered)
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const unsigned o = __builtin_bit_cast(unsigned, shfl_xor_f32(mf, x));
            m = o > m ? o : m;
            mf = __builtin_bit_cast(float, m);
        }
        if ((tid & 63) == 0 && m != 0) atomic_max_agent(a.absmax + (long long)mb * a.n_tasks + a.path_task[p], m);
    }
    scatter_span(a.adv + r0, a.adv_in + s0, n, tid);
    scatter_span(a.act + r0 * a.A, a.act_in + s0 * a.A, n * a.A, tid);
    scatter_span(a.mean + r0 * a.A, a.mean_in + s0 * a.A, n * a.A, tid);
    if (a.ls_in) scatter_span(a.ls + r0 * a.A, a.ls_in + s0 * a.A, n * a.A, tid);
}

enum { POINT_REWARD_DENSE = 0, POINT_REWARD_DENSE_SQUARED = 1, POINT_REWARD_SPARSE = 2 };

// |p - c|_2 the way a row-wise 2-norm rounds it (squares, sum, root; no fused multiply-add): the sparse reward compares the
// goal's distance with the corners' distances for EQUALITY, so every distance must come out of the same arithmetic
PROMP_HD double point_distance(double p0, double p1, double c0, double c1) {
#pragma clang fp contract(off)
    const double d0 = p0 - c0, d1 = p1 - c1;
    const double q0 = d0 * d0, q1 = d1 * d1;
    return sqrt(q0 + q1);
}

struct PointRolloutArgs {
    const float* theta_tasks;   // [tasks][Theta]
    int NP, H1, H2;
    int B, T;                   // environments per task, horizon
    const double* goals;        // [tasks][2]
    const double* start;        // [tasks][B][2] initial states
    const float* noise;         // [tasks][B][T][2] standard normals, or NULL: drawn on the device from (seed, stream)
    unsigned long long seed;
    unsigned stream;
    float *obs, *act, *rew, *mean;   // slab rows ((task * B + b) * T + t)
    float* old_ls;              // [tasks][2] log_std reported in agent_infos
    int clip_infos;
    float min_log_std;
    double normalization_scale; // the normalize wrapper's policy-side action box half-width (10); 0: bare environment
    double max_step;            // the environment's action box [-max_step, max_step] (0.2)
    int reward_type;
    double sparse_radius;       // 0.5
};

// one coordinate of the move a policy action asks for
PROMP_DEV double point_env_move(const PointRolloutArgs& a, float act) {
    const double lb = -a.max_step, ub = a.max_step, sc = a.normalization_scale;
    const double e = sc > 0.0 ? lb + ((double)act + sc) * (ub - lb) / (2.0 * sc) : (double)act;
    return fmin(fmax(e, lb), ub);
}

// one step of the normalised point environment: the state advances in place, the reward comes back
PROMP_DEV double point_env_step(const PointRolloutArgs& a, double& s0, double& s1, double g0, double g1, float a0, float a1) {
    // normalize wrapper: lb + (a + s) (ub - lb) / (2 s), clipped to the action box; then the environment's own clip
    // (same bounds).  Same operation order as normalized_env.py:113-114 so that float64 states agree bit for bit.
    const double d0 = point_env_move(a, a0), d1 = point_env_move(a, a1);
    const double p0 = s0, p1 = s1;
    s0 += d0;
    s1 += d1;
    const double dist = point_distance(s0, s1, g0, g1);
    double r;
    if (a.reward_type == POINT_REWARD_DENSE) {
        r = -dist;
    } else if (a.reward_type == POINT_REWARD_DENSE_SQUARED) {
        r = -(dist * dist);
    } else {
        r = 0.0;
        if (fabs(s0) + fabs(s1) >= a.sparse_radius) {        // left the start region (L1 norm)
            double nearest = dist;
            for (int c = 0; c < 4; ++c) {                    // corners (-2,-2), (2,-2), (-2,2), (2,2)
                const double c0 = (c & 1) ? 2.0 : -2.0, c1 = (c & 2) ? 2.0 : -2.0;
                nearest = fmin(nearest, point_distance(s0, s1, c0, c1));
            }
            if (dist == nearest) r = point_distance(p0, p1, g0, g1) - dist;   // progress
        }
    }
    return r;
}

// grid = tasks, block = 64
__global__ void __launch_bounds__(64) k_point_rollout(PointRolloutArgs a) {
    const int task = blockIdx.x;
    const float* th = a.theta_tasks + (long long)task * a.NP;
    const int oS = a.NP - 2;
    const float ls0 = th[oS], ls1 = th[oS + 1];
    if (threadIdx.x == 0) {
        a.old_ls[task * 2 + 0] = a.clip_infos ? fmaxf(ls0, a.min_log_std) : ls0;
        a.old_ls[task * 2 + 1] = a.clip_infos ? fmaxf(ls1, a.min_log_std) : ls1;
    }
    const float sd0 = expf(ls0), sd1 = expf(ls1);
    const double g0 = a.goals[task * 2], g1 = a.goals[task * 2 + 1];
    for (int b = threadIdx.x; b < a.B; b += 64) {
        const long long env = (long long)task * a.B + b;
        double s0 = a.start[env * 2], s1 = a.start[env * 2 + 1];
        for (int t = 0; t < a.T; ++t) {
            const long long row = env * a.T + t;
            const float o[2] = {(float)s0, (float)s1};
            float m[2], n0, n1;
            mlp_mean(th, o, 2, 2, a.H1, a.H2, m);
            if (a.noise != nullptr) {
                n0 = a.noise[row * 2];
                n1 = a.noise[row * 2 + 1];
            } else {
                action_noise(a.seed, (unsigned long long)row, 0u, a.stream, n0, n1);
            }
            const float a0 = fmaf(sd0, n0, m[0]), a1 = fmaf(sd1, n1, m[1]);
            a.obs[row * 2] = o[0];  a.obs[row * 2 + 1] = o[1];
            a.mean[row * 2] = m[0];  a.mean[row * 2 + 1] = m[1];
            a.act[row * 2] = a0;  a.act[row * 2 + 1] = a1;
            const double r = point_env_step(a, s0, s1, g0, g1, a0, a1);
            a.rew[row] = (float)r;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The point-mass FAMILY: the reference's other two fixed-horizon meta-environments with corner goals, beside the corner
// environment above.  Per-task parameters [task_dim], per-environment start state [state_dim], obs_dim = state_dim:
//   POINT_KIND_CORNER   (2, 2)  point_env_step above
//   POINT_KIND_WALLS    (6, 2)  envs/point_envs/point_env_2d_walls.py:36-51, 71-83: task = (goal, gap_1, gap_2); two circular walls
//                               of radius 1 and 2, each open within distance 1 of its gap.  The reward is taken on the state
//                               BEFORE a wall acts.  sparse: the progress towards the goal within sparse_radius of it; outside
//                               the reference returns None, which no sampler can sum: 0.0 here.
//   POINT_KIND_MOMENTUM (2, 4)  envs/point_envs/point_env_2d_momentum.py:36-42, 63-71: the action accelerates, state = (position,
//                               velocity) and both are observed.  sparse: max(sparse_radius - |s' - g|, 0).
// Neither ends an episode (done = False in both).  State, projection and reward stay in double: a projected state has norm
// 1 - ~1e-6, which the next step's |p| < 1 must see.
// The mean network of walls and momentum evaluates its hidden units with tanhf, not fast_tanh: an action inside the bare
// environment's box enters momentum's velocity at gain 1 and its position with weights T, T - 1, ..., so fast_tanh's absolute error
// (~1e-7 per unit, a few 1e-7 in the mean) came out as 4e-6 in the observations after 8 steps.  Corner keeps fast_tanh: it is
// k_point_rollout bit for bit.
// ---------------------------------------------------------------------------------------------
enum { POINT_KIND_CORNER = 0, POINT_KIND_WALLS = 1, POINT_KIND_MOMENTUM = 2 };

struct PointFamilyArgs {
    PointRolloutArgs p;        // goals: the task parameters [tasks][task_dim]; start: [tasks][B][state_dim]
    int kind, task_dim, state_dim;
};

// tp = (goal, gap_1, gap_2)
PROMP_DEV double walls_env_step(const PointRolloutArgs& a, double& s0, double& s1, const double* tp, float a0, float a1) {
    const double p0 = s0, p1 = s1;
    double n0 = p0 + point_env_move(a, a0), n1 = p1 + point_env_move(a, a1);
    const double dist = point_distance(n0, n1, tp[0], tp[1]);
    double r;
    if (a.reward_type == POINT_REWARD_DENSE) r = -dist;
    else if (a.reward_type == POINT_REWARD_DENSE_SQUARED) r = -(dist * dist);
    else r = dist < a.sparse_radius ? point_distance(p0, p1, tp[0], tp[1]) - dist : 0.0;
    const double before = point_distance(p0, p1, 0.0, 0.0), after = point_distance(n0, n1, 0.0, 0.0);
    if (before < 1.0 && after > 1.0) {
        if (point_distance(n0, n1, tp[2], tp[3]) > 1.0) {
            const double den = after + 1e-6;
            n0 /= den;
            n1 /= den;
        }
    } else if (before < 2.0 && after > 2.0) {
        if (point_distance(n0, n1, tp[4], tp[5]) > 1.0) {
            const double den = 0.5 * after + 1e-6;
            n0 /= den;
            n1 /= den;
        }
    }
    s0 = n0;
    s1 = n1;
    return r;
}

// s = (position, velocity)
PROMP_DEV double momentum_env_step(const PointRolloutArgs& a, double* s, double g0, double g1, float a0, float a1) {
    s[2] += point_env_move(a, a0);
    s[3] += point_env_move(a, a1);
    s[0] += s[2];
    s[1] += s[3];
    const double dist = point_distance(s[0], s[1], g0, g1);
    if (a.reward_type == POINT_REWARD_DENSE) return -dist;
    if (a.reward_type == POINT_REWARD_DENSE_SQUARED) return -(dist * dist);
    return fmax(a.sparse_radius - dist, 0.0);
}

// s [state_dim] advances in place
PROMP_DEV double point_family_step(const PointFamilyArgs& f, double* s, const double* tp, float a0, float a1) {
    if (f.kind == POINT_KIND_WALLS) return walls_env_step(f.p, s[0], s[1], tp, a0, a1);
    if (f.kind == POINT_KIND_MOMENTUM) return momentum_env_step(f.p, s, tp[0], tp[1], a0, a1);
    return point_env_step(f.p, s[0], s[1], tp[0], tp[1], a0, a1);
}

// grid = tasks, block = 64: k_point_rollout for any kind.  DEVICE_START: the initial states are point_start_state's under row = env
// (a.start is not read); false: the table, and bx is not read
template <bool DEVICE_START>
__global__ void __launch_bounds__(64) k_point_family_rollout(PointFamilyArgs f, PointStartBox bx) {
    const PointRolloutArgs& a = f.p;
    const int task = blockIdx.x, O = f.state_dim;
    const float* th = a.theta_tasks + (long long)task * a.NP;
    const int oS = a.NP - 2;
    const float ls0 = th[oS], ls1 = th[oS + 1];
    if (threadIdx.x == 0) {
        a.old_ls[task * 2 + 0] = a.clip_infos ? fmaxf(ls0, a.min_log_std) : ls0;
        a.old_ls[task * 2 + 1] = a.clip_infos ? fmaxf(ls1, a.min_log_std) : ls1;
    }
    const float sd0 = expf(ls0), sd1 = expf(ls1);
    const double* tp = a.goals + (long long)task * f.task_dim;
    for (int b = threadIdx.x; b < a.B; b += 64) {
        const long long env = (long long)task * a.B + b;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (DEVICE_START) point_start_state(bx, a.stream, (unsigned long long)env, O, s);
        else
        for (int k = 0; k < O; ++k) s[k] = a.start[env * O + k];
        for (int t = 0; t < a.T; ++t) {
            const long long row = env * a.T + t;
            float o[4], m[2], n0, n1;
            for (int k = 0; k < O; ++k) o[k] = (float)s[k];
            if (f.kind == POINT_KIND_CORNER) mlp_mean(th, o, O, 2, a.H1, a.H2, m);
            else mlp_mean_t<true>(th, o, O, 2, a.H1, a.H2, m);
            if (a.noise != nullptr) {
                n0 = a.noise[row * 2];
                n1 = a.noise[row * 2 + 1];
            } else {
                action_noise(a.seed, (unsigned long long)row, 0u, a.stream, n0, n1);
            }
            const float a0 = fmaf(sd0, n0, m[0]), a1 = fmaf(sd1, n1, m[1]);
            for (int k = 0; k < O; ++k) a.obs[row * O + k] = o[k];
            a.mean[row * 2] = m[0];  a.mean[row * 2 + 1] = m[1];
            a.act[row * 2] = a0;  a.act[row * 2 + 1] = a1;
            const double r = point_family_step(f, s, tp, a0, a1);
            a.rew[row] = (float)r;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Collections whose episodes END EARLY, without a host loop (samplers/meta_sampler.py:87-130 + vectorized_env_executor.py:25-52 of
// the reference: an environment that reports `done`, or whose episode has reached max_path_length, is reset and keeps collecting;
// collection stops at the first vectorised step after which total_samples steps belong to finished episodes, all episodes that end
// at that step count, and the ones still running are dropped).  Four phases, separate launches on one stream, no workgroup waits
// for another, every loop bounded by a launch argument:
//   k_point_collect / k_gen_point_collect   every environment runs max_steps vectorised steps; step s files float32(state), mean,
//                                           action and reward under the staging row (s, env) = s * n_envs + env -- the rows
//                                           promp_policy_step files in ragged mode, the Philox counter included -- and
//                                           end_len[s][env] = the length of the episode that ends with this step, or 0
//   k_collect_stop                          per-step sums of end_len, their running total, the stop step s*
//   k_collect_tables (count, then write)    per task, (env, first step, length) of every episode that ends at a step <= s*, in the
//                                           reference's order: step-major, environment-minor; k_collect_offsets between the two
//                                           turns the tasks' counts into task_path_offsets
//   k_gather_paths                          staging rows -> slab rows, rewards included
// k_point_norm_collect / k_gen_point_norm_collect are the first phase under the normalize wrapper's running observation / reward
// normalisation, k_point_norm_commit its last (below, at PointNormArgs).
// The fourth kind of the family ends episodes:
//   POINT_KIND_GOAL     (2, 2)  envs/point_envs/point_env_2d.py (= corner_goals_point_env_2d.py) and point_env_2d_v2.py:
//                               s' = s + clip(e, -max_step, max_step), reward -|s' - goal|, done = |s'_0| < done_radius and
//                               |s'_1| < done_radius: the box around the ORIGIN in both classes (point_env_2d_v2.py:52-56 tests the
//                               origin although its reward looks at the goal).  point_env_2d.py's reward -|s'| is goal (0, 0):
//                               (0 - x)^2 and x^2 are the same bits.  tanhf in the mean network, as walls and momentum.
// Kinds 0..2 go through point_family_step and never report done: their episodes end by max_path_length alone.
// ---------------------------------------------------------------------------------------------
enum { POINT_KIND_GOAL = 3 };

struct PointCollectArgs {
    PointFamilyArgs f;         // p.obs / act / mean: the staging rows; p.start: [max_steps][n_envs][state_dim]; p.noise: [max_steps][n_envs][2]
                               // or NULL; p.B: environments per task; p.T unused
    float* rew_stage;          // [max_steps][n_envs]
    int* end_len;              // [max_steps][n_envs]
    int max_steps, max_path_length, n_envs;
    double done_radius;
};

// one step of any kind: s advances in place, the reward comes back, done says whether the environment ended the episode
PROMP_DEV double point_collect_step(const PointCollectArgs& c, double* s, const double* tp, float a0, float a1, bool& done) {
    if (c.f.kind != POINT_KIND_GOAL) {
        done = false;
        return point_family_step(c.f, s, tp, a0, a1);
    }
    s[0] += point_env_move(c.f.p, a0);
    s[1] += point_env_move(c.f.p, a1);
    done = fabs(s[0]) < c.done_radius && fabs(s[1]) < c.done_radius;
    return -point_distance(s[0], s[1], tp[0], tp[1]);
}

// grid = tasks, block = 64: one thread per environment.  Consecutive lanes are consecutive environments of one staging step, so
// the stores of a step coalesce.  Every lane runs max_steps trips; an episode's end is a select on the state, not a branch.
// DEVICE_START: every reset() is point_start_state's under the row the table would hold it in, drawn when an episode ends
template <bool DEVICE_START>
__global__ void __launch_bounds__(64) k_point_collect(PointCollectArgs c, PointStartBox bx) {
    const PointFamilyArgs& f = c.f;
    const PointRolloutArgs& a = f.p;
    const int task = blockIdx.x, O = f.state_dim;
    const float* th = a.theta_tasks + (long long)task * a.NP;
    const int oS = a.NP - 2;
    const float ls0 = th[oS], ls1 = th[oS + 1];
    if (threadIdx.x == 0) {
        a.old_ls[task * 2 + 0] = a.clip_infos ? fmaxf(ls0, a.min_log_std) : ls0;
        a.old_ls[task * 2 + 1] = a.clip_infos ? fmaxf(ls1, a.min_log_std) : ls1;
    }
    const float sd0 = expf(ls0), sd1 = expf(ls1);
    const double* tp = a.goals + (long long)task * f.task_dim;
    for (int b = threadIdx.x; b < a.B; b += 64) {
        const long long env = (long long)task * a.B + b;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (DEVICE_START) point_start_state(bx, a.stream, (unsigned long long)env, O, s);
        else
        for (int k = 0; k < O; ++k) s[k] = a.start[env * O + k];
        int len = 0;
        for (int st = 0; st < c.max_steps; ++st) {
            const long long row = (long long)st * c.n_envs + env;
            float o[4], m[2], n0, n1;
            for (int k = 0; k < O; ++k) o[k] = (float)s[k];
            if (f.kind == POINT_KIND_CORNER) mlp_mean(th, o, O, 2, a.H1, a.H2, m);
            else mlp_mean_t<true>(th, o, O, 2, a.H1, a.H2, m);
            if (a.noise != nullptr) {
                n0 = a.noise[row * 2];
                n1 = a.noise[row * 2 + 1];
            } else {
                action_noise(a.seed, (unsigned long long)row, 0u, a.stream, n0, n1);
            }
            const float a0 = fmaf(sd0, n0, m[0]), a1 = fmaf(sd1, n1, m[1]);
            for (int k = 0; k < O; ++k) a.obs[row * O + k] = o[k];
            a.mean[row * 2] = m[0];  a.mean[row * 2 + 1] = m[1];
            a.act[row * 2] = a0;  a.act[row * 2 + 1] = a1;
            bool done;
            const double r = point_collect_step(c, s, tp, a0, a1, done);
            ++len;
            const bool end = done || len >= c.max_path_length;
            c.rew_stage[row] = (float)r;
            c.end_len[row] = end ? len : 0;
            len = end ? 0 : len;
            // the next episode's reset() (a uniform condition; the reload is a select).  Asking for it ahead of the network was
            // tried and is slower (profiles/point_collect_timing.txt): the extra array is indexed by the runtime state width
            if constexpr (DEVICE_START) {
                // drawn only by the lanes whose episode ends: a wave none of whose episodes ends skips the block (a select
                // would run the ten Philox rounds in every step; profiles/point_start_timing.txt)
                if (end && st + 1 < c.max_steps) point_start_state(bx, a.stream, (unsigned long long)(row + c.n_envs), O, s);
            } else
            if (st + 1 < c.max_steps) {
                const long long nxt = row + c.n_envs;
                for (int k = 0; k < O; ++k) {
                    const double fresh = a.start[nxt * O + k];
                    s[k] = end ? fresh : s[k];
                }
            }
        }
    }
}

// ---- running observation / reward normalisation (envs/normalized_env.py:73-123 of the reference: normalize(env, normalize_obs=True,
// normalize_reward=True)).  Every environment owns one wrapper state -- obs_mean [O], obs_var [O], rew_mean, rew_var, float64, 2 O + 2
// values -- that lives in the context across calls (promp_point_norm_set / _get).  Inside a collection it sits in registers of the
// lane that owns the environment and is updated once per sample, in the wrapper's order:
//   reset()            the raw start state updates the obs moments; the policy sees float32((x - mean) / (sqrt(var) + 1e-8))
//   step()             the bare environment steps on its RAW state; the raw next observation (the terminal one included) updates the obs
//                      moments, the raw reward the reward moments; the stored reward is float32(r / (sqrt(rew_var) + 1e-8))
//   episode end        reset() at once: start[s + 1][env] updates the obs moments (vectorized_env_executor.py:45-52), also at the
//                      step collection stops at -- the start table has max_steps + 1 rows
// The state a call leaves is the state after the stop step s*, which only k_collect_stop knows: every step stages the moments behind
// its events into norm.stage [max_steps][2 O + 2][n_envs] (environment-minor: a wave's stores coalesce), and k_point_norm_commit
// copies row s* into the persistent buffer once the host has accepted the collection.  Steps beyond s* leave no trace.
struct PointNormArgs {
    int normalize_obs, normalize_reward;
    double obs_alpha, reward_alpha;
    const double* moments;     // [n_envs][2 O + 2]: obs_mean, obs_var, rew_mean, rew_var (read at entry)
    double* stage;             // [max_steps][2 O + 2][n_envs]
};
struct PointNormState {
    double om[4], ov[4], rm, rv;
};

// one sample: mean <- (1 - alpha) mean + alpha x; var <- (1 - alpha) var + alpha (x - NEW mean)^2, every product rounded on its own
// (normalized_env.py:73-81 in NumPy's float64)
PROMP_HD void point_norm_update(double& mean, double& var, double x, double alpha) {
#pragma clang fp contract(off)
    const double keep = 1.0 - alpha;
    const double km = keep * mean, ax = alpha * x;
    const double m = km + ax;
    const double d = x - m;
    const double q = d * d;
    const double kv = keep * var, aq = alpha * q;
    mean = m;
    var = kv + aq;
}
PROMP_DEV void point_norm_see(const PointNormArgs& n, PointNormState& w, const double* s, int O) {
    for (int k = 0; k < O; ++k) point_norm_update(w.om[k], w.ov[k], s[k], n.obs_alpha);
}
// what the policy is handed for the raw state s
PROMP_DEV float point_norm_obs(const PointNormArgs& n, const PointNormState& w, const double* s, int k) {
    if (n.normalize_obs) return (float)((s[k] - w.om[k]) / (sqrt(w.ov[k]) + 1e-8));
    return (float)s[k];
}
// entry: the persistent state, then the first reset()
PROMP_DEV void point_norm_enter(const PointNormArgs& n, PointNormState& w, const double* s, int O, long long env) {
    const double* m = n.moments + env * (2 * O + 2);
    for (int k = 0; k < O; ++k) {
        w.om[k] = m[k];
        w.ov[k] = m[O + k];
    }
    w.rm = m[2 * O];
    w.rv = m[2 * O + 1];
    if (n.normalize_obs) point_norm_see(n, w, s, O);
}

// The tail of vectorised step st of environment env under the wrapper, shared by k_point_norm_collect and k_gen_point_norm_collect:
// k_point_collect's tail (the environment steps on (a0, a1), the step's reward and end_len are filed under `row`, the next
// episode's reset() is taken from the start table) with the wrapper's events in it, and the moments staged behind them.
template <bool DEVICE_START>
PROMP_DEV void point_norm_collect_tail(const PointCollectArgs& c, const PointNormArgs& n, const PointStartBox& bx, PointNormState& w, double* s,
                                       const double* tp, float a0, float a1, long long row, long long env, int st, int& len) {
    const PointRolloutArgs& a = c.f.p;
    const int O = c.f.state_dim;
    bool done;
    double r = point_collect_step(c, s, tp, a0, a1, done);
    ++len;
    const bool end = done || len >= c.max_path_length;
    if (n.normalize_obs) point_norm_see(n, w, s, O);              // the raw next observation, terminal or not
    if (n.normalize_reward) {
        point_norm_update(w.rm, w.rv, r, n.reward_alpha);
        r = r / (sqrt(w.rv) + 1e-8);
    }
    c.rew_stage[row] = (float)r;
    c.end_len[row] = end ? len : 0;
    len = end ? 0 : len;
    const long long nxt = row + c.n_envs;                         // (the table has a row behind the last step)
    if constexpr (DEVICE_START) {
        // drawn every step and selected, as the table reload is (the row behind the last step too): under the wrapper the draw
        // beneath `if (end)`, which the plain kernels have, measured 2 % slower (profiles/point_start_timing.txt)
        double fresh[4] = {0.0, 0.0, 0.0, 0.0};
        point_start_state(bx, a.stream, (unsigned long long)nxt, O, fresh);
        for (int k = 0; k < O; ++k) s[k] = end ? fresh[k] : s[k];
    } else
    for (int k = 0; k < O; ++k) {
        const double fresh = a.start[nxt * O + k];
        s[k] = end ? fresh : s[k];
    }
    if (n.normalize_obs && end) point_norm_see(n, w, s, O);       // reset() at once, at the stop step too
    const int W = 2 * O + 2;
    double* out = n.stage + (long long)st * W * c.n_envs + env;
    for (int k = 0; k < O; ++k) {
        out[(long long)k * c.n_envs] = w.om[k];
        out[(long long)(O + k) * c.n_envs] = w.ov[k];
    }
    out[(long long)(2 * O) * c.n_envs] = w.rm;
    out[(long long)(2 * O + 1) * c.n_envs] = w.rv;
}

struct PointNormCollectArgs {
    PointCollectArgs c;        // p.start: [max_steps + 1][n_envs][state_dim]
    PointNormArgs n;
};
// grid = tasks, block = 64: k_point_collect under the normalize wrapper's running moments (a sibling: k_point_collect itself is
// untouched, so the plain collection is the same machine code as before)
template <bool DEVICE_START>
__global__ void __launch_bounds__(64) k_point_norm_collect(PointNormCollectArgs g, PointStartBox bx) {
    const PointCollectArgs& c = g.c;
    const PointNormArgs& n = g.n;
    const PointFamilyArgs& f = c.f;
    const PointRolloutArgs& a = f.p;
    const int task = blockIdx.x, O = f.state_dim;
    const float* th = a.theta_tasks + (long long)task * a.NP;
    const int oS = a.NP - 2;
    const float ls0 = th[oS], ls1 = th[oS + 1];
    if (threadIdx.x == 0) {
        a.old_ls[task * 2 + 0] = a.clip_infos ? fmaxf(ls0, a.min_log_std) : ls0;
        a.old_ls[task * 2 + 1] = a.clip_infos ? fmaxf(ls1, a.min_log_std) : ls1;
    }
    const float sd0 = expf(ls0), sd1 = expf(ls1);
    const double* tp = a.goals + (long long)task * f.task_dim;
    for (int b = threadIdx.x; b < a.B; b += 64) {
        const long long env = (long long)task * a.B + b;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (DEVICE_START) point_start_state(bx, a.stream, (unsigned long long)env, O, s);
        else
        for (int k = 0; k < O; ++k) s[k] = a.start[env * O + k];
        PointNormState w;
        point_norm_enter(n, w, s, O, env);
        int len = 0;
        for (int st = 0; st < c.max_steps; ++st) {
            const long long row = (long long)st * c.n_envs + env;
            float o[4], m[2], n0, n1;
            for (int k = 0; k < O; ++k) o[k] = point_norm_obs(n, w, s, k);
            if (f.kind == POINT_KIND_CORNER) mlp_mean(th, o, O, 2, a.H1, a.H2, m);
            else mlp_mean_t<true>(th, o, O, 2, a.H1, a.H2, m);
            if (a.noise != nullptr) {
                n0 = a.noise[row * 2];
                n1 = a.noise[row * 2 + 1];
            } else {
                action_noise(a.seed, (unsigned long long)row, 0u, a.stream, n0, n1);
            }
            const float a0 = fmaf(sd0, n0, m[0]), a1 = fmaf(sd1, n1, m[1]);
            for (int k = 0; k < O; ++k) a.obs[row * O + k] = o[k];
            a.mean[row * 2] = m[0];  a.mean[row * 2 + 1] = m[1];
            a.act[row * 2] = a0;  a.act[row * 2 + 1] = a1;
            point_norm_collect_tail<DEVICE_START>(c, n, bx, w, s, tp, a0, a1, row, env, st, len);
        }
    }
}

// the wrapper state a collection leaves: row s* of the staged moments -> the persistent buffer.  Launched only after the host has
// accepted the collection.  grid = ceil(n_envs / 256), block = 256: one thread per environment
struct PointNormCommitArgs {
    const double* stage;       // [max_steps][W][n_envs]
    const long long* stop;     // k_collect_stop's out
    double* moments;           // [n_envs][W]
    int W, n_envs, max_steps;
};
__global__ void __launch_bounds__(256) k_point_norm_commit(PointNormCommitArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    const long long s = a.stop[0];
    if (env >= a.n_envs || s < 0 || s >= a.max_steps) return;
    const double* in = a.stage + s * a.W * a.n_envs + env;
    for (int j = 0; j < a.W; ++j) a.moments[(long long)env * a.W + j] = in[(long long)j * a.n_envs];
}

// out[0] = s*, the first step at which the running total of finished-episode steps reaches total_samples (-1: max_steps did not
// reach it), out[1] = that total at s* (the rows; all episodes ending at s* count, so it may exceed total_samples), out[2] = 1 if
// max_steps did not reach total_samples.  step_sum [max_steps] is scratch and a by-product.
struct CollectStopArgs {
    const int* end_len;        // [max_steps][n_envs]
    int* step_sum;             // [max_steps]
    long long* out;            // [3]
    int max_steps, n_envs;
    long long total_samples;
};
// grid = 1, block = 256: wave w sums the steps w, w + 4, ...; then one thread walks the max_steps sums
__global__ void __launch_bounds__(256) k_collect_stop(CollectStopArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < a.max_steps; s += 4) {
        double n = 0.0;                                            // (sums of int32 lengths: exact in double)
        for (int e = lane; e < a.n_envs; e += 64) n += (double)a.end_len[(long long)s * a.n_envs + e];
        n = wave_sum_f64(n);
        if (lane == 0) a.step_sum[s] = (int)n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = 0, rows = 0;
        int stop = -1;
        for (int s = 0; s < a.max_steps; ++s) {
            total += a.step_sum[s];
            const bool first = stop < 0 && total >= a.total_samples;
            stop = first ? s : stop;
            rows = first ? total : rows;
        }
        a.out[0] = stop;
        a.out[1] = rows;
        a.out[2] = stop < 0 ? 1 : 0;
    }
}

struct CollectTablesArgs {
    const int* end_len;        // [max_steps][n_envs]
    const long long* stop;     // k_collect_stop's out
    int* task_count;           // [tasks]: written when write == 0
    const int* task_path_offsets;   // [tasks + 1]: read when write == 1
    int *path_env, *path_start, *path_len;   // [max_paths]
    int B, max_steps, n_envs, n_tasks, max_paths, write;
};
// exclusive prefix count of a flag over the wave's lanes, and the wave's total (Hillis-Steele over lane shuffles)
PROMP_DEV int wave_prefix_count(bool flag, int lane, int& total) {
    double v = flag ? 1.0 : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = shfl_idx_f64(v, lane >= d ? lane - d : lane);
        v += lane >= d ? o : 0.0;
    }
    total = (int)shfl_idx_f64(v, 63);
    return (int)v - (flag ? 1 : 0);
}
// grid = tasks, block = 64 (one wave): steps 0..s* in order, within a step the task's environments in index order, 64 at a time.
// write == 0 counts the task's paths; write == 1 files them behind task_path_offsets[task] (nothing if they exceed max_paths).
__global__ void __launch_bounds__(64) k_collect_tables(CollectTablesArgs a) {
    const int task = blockIdx.x, lane = threadIdx.x;
    const int s_stop = (int)a.stop[0];
    const int base = a.write ? a.task_path_offsets[task] : 0;
    const bool fits = a.write && a.task_path_offsets[a.n_tasks] <= a.max_paths;
    int count = 0;
    for (int s = 0; s < a.max_steps; ++s) {
        if (s > s_stop) break;                                     // (uniform)
        for (int b0 = 0; b0 < a.B; b0 += 64) {
            const int b = b0 + lane, env = task * a.B + b;
            const int len = b < a.B ? a.end_len[(long long)s * a.n_envs + env] : 0;
            int total;
            const int pos = base + count + wave_prefix_count(len > 0, lane, total);
            if (fits && len > 0) {
                a.path_env[pos] = env;
                a.path_start[pos] = s - len + 1;
                a.path_len[pos] = len;
            }
            count += total;
        }
    }
    if (!a.write && lane == 0) a.task_count[task] = count;
}
// grid = 1, block = 64: task_path_offsets [tasks + 1] from the tasks' counts
__global__ void __launch_bounds__(64) k_collect_offsets(const int* task_count, int* task_path_offsets, int n_tasks) {
    if (threadIdx.x != 0) return;
    int n = 0;
    for (int i = 0; i < n_tasks; ++i) {
        task_path_offsets[i] = n;
        n += task_count[i];
    }
    task_path_offsets[n_tasks] = n;
}

// ---- collections whose environment lives on the device (promp_file_step_dev) -------------------------------------------------
// The outcome of vectorised step s of every environment, filed where k_point_collect files its own: the reward under (s, env) of the
// staged rewards, the length of an episode that ends at s under (s, env) of end_len (0: still running).  ep_len [n_envs] is the
// length of every environment's episode in progress; the launch of s == 0 starts it from zero.
//   len = ep_len[env] + 1;  end = (done && done[env]) || len == max_path_length
// Fixed horizon (promp_begin_rollout): end_len == nullptr; the reward goes to slab row env * T + s (rew_env_stride = T), `done` is
// not read and every environment reports fixed_end (s == T - 1).
struct FileStepArgs {
    const float* rewards;        // [n_envs]
    const unsigned char* done;   // [n_envs] or nullptr
    unsigned char* ended_out;    // [n_envs] or nullptr
    float* rew_out;              // where environment 0's reward of this step goes; environment e: + e * rew_env_stride
    long long rew_env_stride;
    int* end_len;                // row s of end_len [max_steps][n_envs], or nullptr: fixed horizon
    int* ep_len;                 // [n_envs] (ragged collections only)
    int n_envs, s, max_path_length, fixed_end;
};
// grid = ceil(n_envs / 256), block = 256: one thread per environment, consecutive lanes = consecutive environments
__global__ void __launch_bounds__(256) k_file_step(FileStepArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n_envs) return;
    a.rew_out[(long long)env * a.rew_env_stride] = a.rewards[env];
    bool end = a.fixed_end != 0;
    if (a.end_len != nullptr) {
        const int len = (a.s == 0 ? 0 : a.ep_len[env]) + 1;
        end = (a.done != nullptr && a.done[env] != 0) || len == a.max_path_length;
        a.end_len[env] = end ? len : 0;
        a.ep_len[env] = end ? 0 : len;
    }
    if (a.ended_out != nullptr) a.ended_out[env] = end ? 1 : 0;
}
