// promp_kernels_sample.h -- sample processing on the device (reference rows a1-a7), FP64 like the
// reference (SciPy lfilter / NumPy lstsq compute in float64).
//
// The kernels, in launch order (sample_plan() in promp_plan.h decides which of the Gram / fit kernels a call launches; D + 1 =
// the feature columns and the target, NBLK = its blocks of 16):
//   k_returns        per path  R[t] = r[t] + g R[t+1], per-path sums          utils/utils.py:74-81, samplers/base.py:103-104
//                    every call
//   k_dice_scan      per path  DiCE's suffix / prefix sums of the row weights  meta_algos/dice_maml.py:39-45, 245-258
//                    promp_set_dice_rewards (mode 0) and the DICE curvature pass (mode 1), not process_samples
//   k_gram<NBLK>     per work item  partial [Phi R]^T [Phi R], wave-private tiles  baselines/linear_baseline.py:66-67, 101-106
//                    LinearFeatureBaseline obs_dim <= 32 (NBLK <= 5), LinearTimeBaseline (NBLK = 1)
//   k_gram_wide      the same, one shared tile, waves own runs of the block-pair list
//                    obs_dim 33-93 (NBLK <= 12), and wider with PROMP_GRAM_UNTILED=1
//   k_gram_tiled     the same, a wave owns a square of 3 x 3 blocks, operands reused in registers
//                    obs_dim >= 94 (NBLK >= 13: Ant 15 blocks, Humanoid 48)
//   k_fit_wave<DT>   per task  sum the partials, (G + reg I) w = Phi^T R in ONE wave, NaN retry  baselines/linear_baseline.py:68-77
//                    D + 1 <= 64 (DT = 12, 45, 48, 64: obs_dim <= 29, LinearTimeBaseline)
//   k_fit            the same solve, one workgroup, matrices in LDS
//                    obs_dim 30-32 (D + 1 = 65..69)
//   k_gram_sum_wide  per task  sum the partials into G and the work matrix in global memory
//                    obs_dim >= 33, in front of
//   k_fit_wide<NB>   the same solve, blocked right-looking Cholesky, panels of NB = 32 (16: D > ~580) columns through LDS
//                    obs_dim >= 33; alone for D < 400 (PROMP_FIT_ONE_LAUNCH=1: always), else only the retries behind
//   k_fitw_panel<NB>, k_fitw_update<NB>, k_fitw_back<NB>   the same factorisation, one launch per phase
//                    D >= 400 (Humanoid)
//   k_gae            per path  b = Phi w ; delta ; GAE scan ; moments    baselines/linear_baseline.py:17-33, samplers/base.py:151-162
//                    every call (ZeroBaseline: b = 0)
//   k_normalize      per work item  (adv - mean) / (std + 1e-8) [, shift > 0]  utils/utils.py:59-71
//                    every call (pad_length: the statistics of the zero-padded array)
//   k_dice_targets, k_dice_adjust, k_dice_finish   per path  r_t gamma^t ; y - Phi w, moments ; normalise over the padded array,
//                    DiCE rewards and their suffix sums    samplers/dice_sample_processor.py:96-191
//                    promp_process_samples_dice, around the same Gram / fit kernels
// What several of them share is written once, in front of its first user: suffix_scan_chunk; linfeat_obs / linfeat_row_tail (the
// feature row); tri_pair_blocks / tri_pair_index / gram_store_block / gram_scatter_entry (the partial-block layout);
// fit_any_nan; fitw_back_substitute and the chol_* panel steps (the blocked Cholesky).
//
// One wavefront owns one path in the scans: the linear recurrence y[t] = x[t] + c*y[t+1] is a
// 6-step wave-level suffix scan over 64 time steps (weights c, c^2, c^4, ...), chained across
// 64-step chunks from the end of the path with a carry, so ragged path lengths need no padding.
// The Gram matrix runs on the FP64 matrix cores (v_mfma_f64_16x16x4_f64): the target is appended
// to the features as one more column so that Phi^T R falls out of the same product.
#pragma once
#include <utility>
#include "promp_device.h"
#include "promp_plan.h"            // the constants and sizing helpers shared with the host's plan
#include "promp_kernels_policy.h"

enum { BASE_ZERO = 0, BASE_LINFEAT = 1, BASE_LINTIME = 2 };

struct SampleArgs {
    const float* obs;              // [rows][O]
    const float* rew;              // [rows]
    const double* rew64;           // optional [rows]: the rewards in the environment's float64 (else NULL: rew is used)
    const int* path_row_offsets;   // [paths+1]
    const int* path_task;          // [paths]
    const int* row_t;              // [rows] time index inside the path
    const int* task_row_offsets;   // [tasks+1]
    const int* task_path_offsets;  // [tasks+1]
    const WorkItem* work;          // row ranges (multiples of 64 from the task start)
    const int* task_wg_offsets;    // [tasks+1]
    int O, D, kind;
    double gamma, lam, reg;
    int normalize, positive;
    double* ret64;
    float* ret32;
    double* adv64;
    float* adv32;
    double* path_ret0;
    double* path_undisc;
    double* path_rsq;
    double* path_mom;       // [paths][3] sum adv, sum adv^2, min adv
    double* gram_partials;  // [grid][NPAIR*256]
    double* coeffs;         // [tasks][coeff_stride]
    int coeff_stride;
    double* bl64;           // optional [rows]: the baseline predictions Phi.w (LinearBaseline.predict), else NULL
    // statistics over a task's zero-padded [paths, pad_length] array (the DiCE sample processor); 0: over the task's rows
    int pad_length;
    int pad_scale;          // k_normalize: adv32 receives x * rows / (paths * pad_length), the weight of a slab mean
    double* x64;            // optional [rows]: the normalised / shifted values in float64
    double* pad_out;        // optional [tasks]: what a padded zero maps to
    float* dice_rw;         // [rows] k_dice_finish: x * rows / (paths * pad_length)
};

// Suffix scan of one 64-step chunk, a step per lane: y[lane] = sum_{d >= 0, lane + d < 64} c^d x[lane + d] in six shuffle steps
// (weights c, c^2, c^4, ...).  The unweighted instance (c = 1: DiCE's sums) multiplies by nothing.  The caller chains chunks from
// the end of the path: + c^(64 - lane) * carry, carry = the next chunk's lane 0.
template <bool WEIGHTED>
PROMP_DEV double suffix_scan_chunk(double x, int lane, double c = 1.0) {
    double y = x, cc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double up = shfl_down_f64(y, d);
        if (lane + d < 64) y += WEIGHTED ? cc * up : up;
        if (WEIGHTED) cc *= cc;
    }
    return y;
}

// grid = paths, block = 64
__global__ void __launch_bounds__(64) k_returns(SampleArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.path_row_offsets[p], T = a.path_row_offsets[p + 1] - row0;
    const double g = a.gamma;
    const double f = pow(g, (double)(64 - lane));
    double carry = 0.0, usum = 0.0, rsq = 0.0, y0 = 0.0;
    for (int end = T; end > 0; end -= 64) {
        const int t = end - 64 + lane;
        const int rr = row0 + (t >= 0 ? t : 0);
        const double x = (t >= 0) ? (a.rew64 ? a.rew64[rr] : (double)a.rew[rr]) : 0.0;
        double y = suffix_scan_chunk<true>(x, lane, g);
        y += f * carry;
        if (t >= 0) {
            a.ret64[row0 + t] = y;
            a.ret32[row0 + t] = (float)y;
        }
        if (t == 0) y0 = y;
        carry = shfl_idx_f64(y, 0);
        usum += x;
        rsq += x * x;
    }
    usum = wave_sum_f64(usum);
    rsq = wave_sum_f64(rsq);
    y0 = wave_sum_f64(y0);
    if (lane == 0) {
        a.path_ret0[p] = y0;
        a.path_undisc[p] = usum;
        a.path_rsq[p] = rsq;
    }
}

// DiCE weights (meta_algos/dice_maml.py:39-45, 245-258: the magic box couples the time steps of a path).
//   mode 0:  out[t] = sum_{t' >= t} rw[t']                                   (gradient weights w)
//   mode 1:  out[t] = sum_{t' >= t} rw[t'] C[t'],  C[t'] = sum_{t'' <= t'} c[t'']   (Hessian-vector coupling weights u)
// One wave per path, float64 suffix scans in 64-row chunks from the end (suffix_scan_chunk, unweighted); the prefix sum
// is total - suffix + own.  grid = paths, block = 64.
struct DiceScanArgs {
    const int* path_row_offsets;
    const float* rw;       // [rows] adjusted reward * rows / (paths * max_path_length) of every valid row
    const float* c;        // [rows] row tangents (mode 1)
    float* out;            // [rows]
    double* tmp;           // [rows] scratch (mode 1)
    int mode;
};
__global__ void __launch_bounds__(64) k_dice_scan(DiceScanArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.path_row_offsets[p], T = a.path_row_offsets[p + 1] - row0;
    double total = 0.0;
    if (a.mode == 1) {
        double carry = 0.0;
        for (int end = T; end > 0; end -= 64) {
            const int t = end - 64 + lane;
            const double x = (t >= 0) ? (double)a.c[row0 + t] : 0.0;
            const double y = suffix_scan_chunk<false>(x, lane) + carry;
            if (t >= 0) a.tmp[row0 + t] = y;
            carry = shfl_idx_f64(y, 0);
        }
        total = carry;
    }
    double carry = 0.0;
    for (int end = T; end > 0; end -= 64) {
        const int t = end - 64 + lane;
        double x = 0.0;
        if (t >= 0) {
            x = (double)a.rw[row0 + t];
            if (a.mode == 1) x *= total - a.tmp[row0 + t] + (double)a.c[row0 + t];     // C[t]
        }
        const double y = suffix_scan_chunk<false>(x, lane) + carry;
        if (t >= 0) a.out[row0 + t] = (float)y;
        carry = shfl_idx_f64(y, 0);
    }
}

// ---------------------------------------------------------------------------------------------
// The LinearFeatureBaseline feature row (baselines/linear_baseline.py:101-106), one row of [Phi R]:
//   columns 0 .. O-1 clip(obs, -10, 10) | O .. 2O-1 its square | qt .. qt+3 tau, tau^2, tau^3, 1 (tau = t / 100) | D the target
// (qt = 2 O; LinearTimeBaseline: no observation columns, qt = 0).  The reference squares in the observations' own dtype
// (float32), then promotes.  tau * tau * tau associates as (tau tau) tau.
// ---------------------------------------------------------------------------------------------
// one observation entry: the clipped value into row[c], its float32 square into row[c2] (live = false: a row past the chunk's
// last, zeros)
PROMP_DEV void linfeat_obs(float x, bool live, double* row, int c, int c2) {
    const float oc = live ? fminf(fmaxf(x, -10.f), 10.f) : 0.f;
    row[c] = (double)oc;
    row[c2] = (double)(oc * oc);
}
PROMP_DEV double linfeat_tau(int t) { return (double)t / 100.0; }
// a row's tail into the feature row pr (valid = false: a row past the chunk's last, zeros)
PROMP_DEV void linfeat_row_tail(double* pr, int qt, int D, bool valid, int t, double target) {
    const double tau = valid ? linfeat_tau(t) : 0.0;
    pr[qt] = tau;
    pr[qt + 1] = tau * tau;
    pr[qt + 2] = tau * tau * tau;
    pr[qt + 3] = valid ? 1.0 : 0.0;
    pr[D] = valid ? target : 0.0;
}

// ---------------------------------------------------------------------------------------------
// The partial Gram of a work item (gram_partials): [pair][256] doubles.  The D + 1 columns of [Phi R] are cut into n = NBLK
// blocks of 16; pair = the row-major index of block (bi, bj >= bi) in the upper block triangle; entry (i, j) of a block sits at
// 16 i + j.  An FP64 16x16x4 accumulator holds, in lane (kk = lane >> 4, i16 = lane & 15), the entries (kk + 4 r, i16), r = 0..3.
// (k_gram_tiled numbers its squares of bands the same way, n = the number of bands.)
// ---------------------------------------------------------------------------------------------
PROMP_DEV void tri_pair_blocks(int p, int n, int& bi, int& bj) {
    bi = 0;
    int rem = p;
    while (rem >= n - bi) {
        rem -= n - bi;
        ++bi;
    }
    bj = bi + rem;
}
PROMP_DEV int tri_pair_index(int bi, int bj, int n) { return bi * n - bi * (bi - 1) / 2 + (bj - bi); }
// an accumulator into block p of out (global partials, or a wave's LDS slab)
PROMP_DEV void gram_store_block(double* out, int p, const f64x4& acc, int kk, int i16) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[p * 256 + (kk + 4 * r) * 16 + i16] = acc[r];
}
// entry e of the partial layout, summed over the task's work items, into the symmetric (D + 1) x (D + 1) matrix G -- and, WORK,
// into the work matrix Wm = G + reg I of a first factorisation attempt (the ridge term on the D feature rows, not on the target's)
template <bool WORK = false>
PROMP_DEV void gram_scatter_entry(double s, int e, int NBLK, int D, double* G, double* Wm = nullptr, double reg = 0.0) {
    const int DA = D + 1;
    int bi, bj;
    tri_pair_blocks(e >> 8, NBLK, bi, bj);
    const int row = 16 * bi + ((e & 255) >> 4), col = 16 * bj + (e & 15);
    if (row < DA && col < DA) {
        const double diag = (row == col && row < D) ? reg : 0.0;
        G[(size_t)row * DA + col] = s;
        if (WORK) Wm[(size_t)row * DA + col] = s + diag;
        if (bi != bj) {
            G[(size_t)col * DA + row] = s;
            if (WORK) Wm[(size_t)col * DA + row] = s;
        }
    }
}

// k_gram: partial Gram of [Phi R] over a work item's rows, wave-private like the policy passes: every wave builds
// the features of its own 16-row chunks in its own LDS tile and feeds them to v_mfma_f64_16x16x4_f64 (the same
// register is A and B operand of a block pair); no workgroup barrier in the chunk loop.  The waves' blocks are added
// in wave order through LDS slabs at the end.
template <int NBLK>
struct GramCfg {
    static constexpr int NW = (NBLK <= 3) ? 8 : 4;                            // waves per workgroup
    static constexpr int FS = (NBLK % 2 == 1) ? 16 * NBLK : 16 * NBLK + 16;   // feature-tile row stride (doubles)
    static constexpr int NPAIR = NBLK * (NBLK + 1) / 2;
    static constexpr int WAVE_BYTES = 16 * FS * 8 + 16 * 32 * 4 + 2 * 16 * 8;  // Phi | raw obs [16][<=32] | targets | tau
    static constexpr int SLAB_BYTES = NW * NPAIR * 256 * 8;
    static constexpr int SMEM_BYTES = (NW * WAVE_BYTES > SLAB_BYTES) ? NW * WAVE_BYTES : SLAB_BYTES;
};

// grid = work items, block = 64 * GramCfg<NBLK>::NW
#ifdef PROMP_DEV_STAMPS
#define SA_STAMPS unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tph = promp_clock()
#define SA_PHASE(i) do { const unsigned long long now_ = promp_clock(); ph[i] += now_ - tph; tph = now_; } while (0)
#else
#define SA_STAMPS do { } while (0)
#define SA_PHASE(i) do { } while (0)
#endif
template <int NBLK>
__global__ void __launch_bounds__(64 * GramCfg<NBLK>::NW) k_gram(SampleArgs a) {
    SA_STAMPS;
    constexpr int NW = GramCfg<NBLK>::NW, FS = GramCfg<NBLK>::FS, NPAIR = GramCfg<NBLK>::NPAIR, NC = 16 * NBLK;
    PROMP_SMEM_DECL;
    unsigned char* smem = (unsigned char*)PROMP_SMEM_PTR;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, kk = lane >> 4;
    double* Phi = (double*)(smem + (size_t)w * GramCfg<NBLK>::WAVE_BYTES);
    const WorkItem wk = a.work[blockIdx.x];
    const int O = a.O, D = a.D;
    f64x4 acc[NPAIR];
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) acc[p] = zero4d();
    // A chunk's inputs (this lane's share of the [16][O <= 32] observation rows, a row's return and time index) are
    // requested one chunk ahead: the wave walks ~5 chunks and would otherwise sit out a memory round trip in each.
    float xr[8];
    double tr = 0.0;
    int ttr = 0;
    auto request = [&](int base) {
        const bool live = base < wk.row_end;
        const int nrows = !live ? 0 : (wk.row_end - base) < 16 ? (wk.row_end - base) : 16;
        const long long b0 = live ? base : wk.row_begin;          // always a valid row of this work item
        if (a.kind == BASE_LINFEAT) {
            const int lim = nrows * O;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = lane + 64 * u;
                const float x = a.obs[b0 * O + (e < lim ? e : 0)];
                xr[u] = (e < lim) ? x : 0.f;
            }
        }
        if (lane < 16) {
            const int r = lane < nrows ? lane : 0;
            tr = a.ret64[b0 + r];
            ttr = a.row_t[b0 + r];
        }
    };
    // The feature tile is written straight from the registers the request filled: element e = lane + 64 u of the [16][O] chunk is
    // observation c = e mod O of row e / O, and goes to columns c (clipped) and O + c (its square) -- the positions are the same for
    // every chunk.  Lanes 0..15 add their row's time features, the constant and the target.  Columns past D + 1 stay zero.
    int poff[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = lane + 64 * u, r = e / (O > 0 ? O : 1);
        poff[u] = (a.kind == BASE_LINFEAT && e < 16 * O) ? r * FS + (e - r * O) : -1;
    }
    for (int e = lane; e < 16 * FS; e += 64) Phi[e] = 0.0;
    wave_sync();
    const int qt = (a.kind == BASE_LINFEAT) ? 2 * O : 0;        // first of the four time columns (tau, tau^2, tau^3, 1)
    request(wk.row_begin + 16 * w);
    SA_PHASE(0);
    for (int base = wk.row_begin + 16 * w; base < wk.row_end; base += 16 * NW) {
        const int nrows = (wk.row_end - base) < 16 ? (wk.row_end - base) : 16;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (poff[u] >= 0)
                linfeat_obs(xr[u], true, Phi, poff[u], poff[u] + O);       // (rows past the chunk's last arrive as zeros)
        if (lane < 16) linfeat_row_tail(Phi + lane * FS, qt, D, lane < nrows, ttr, tr);
        SA_PHASE(1);
        request(base + 16 * NW);
        wave_sync();
        SA_PHASE(2);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            double av[NBLK];
#pragma unroll
            for (int b = 0; b < NBLK; ++b) av[b] = Phi[(4 * s + kk) * FS + 16 * b + i16];
            int p = 0;
#pragma unroll
            for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
                for (int bj = bi; bj < NBLK; ++bj) {
                    acc[p] = mfma16d(av[bi], av[bj], acc[p]);
                    ++p;
                }
        }
        wave_sync();
        SA_PHASE(3);
    }
    __syncthreads();
    SA_PHASE(4);
    double* S = (double*)smem;   // [NW][NPAIR*256]
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) gram_store_block(S, w * NPAIR + p, acc[p], kk, i16);
    __syncthreads();
    double* out = a.gram_partials + (long long)blockIdx.x * (NPAIR * 256);
    for (int e = tid; e < NPAIR * 256; e += 64 * NW) {
        double t = 0.0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) t += S[ww * NPAIR * 256 + e];
        out[e] = t;
    }
    SA_PHASE(5);
#ifdef PROMP_DEV_STAMPS
    if (blockIdx.x == 0 && tid == 0)
        printf("k_gram cycles (wave 0 of workgroup 0): entry %llu | features %llu | request + sync %llu | products %llu | barrier %llu | slab sums %llu\n",
               ph[0], ph[1], ph[2], ph[3], ph[4], ph[5]);
#endif
}

// "NaN in the solution => reg *= 10" (linear_baseline.py:68-77), the workgroup's vote through an LDS flag: nonzero if any of
// wv[0 .. D) is a NaN.  Every thread of the nt calls it.  The caller has zeroed *flag in front of a barrier that also covers
// wv, and passes another barrier before it zeroes the flag again.  ONE_TRIP: D <= nt, a thread looks at one entry (k_fit: as a
// loop of one trip the vote measured 2.6 us per launch slower at obs_dim 31).
template <bool ONE_TRIP>
PROMP_DEV int fit_any_nan(const double* wv, int D, int* flag, int tid, int nt) {
    if (ONE_TRIP) {
        if (tid < D && wv[tid] != wv[tid]) *flag = 1;
    } else {
        for (int e = tid; e < D; e += nt)
            if (wv[e] != wv[e]) *flag = 1;
    }
    __syncthreads();
    return *flag;
}

// grid = tasks, block = 256.  smem: G[(D+1)^2] + Wm[(D+1)^2] + yv[D+1] + wv[D+1] + dg[D+1]  (doubles)
// The factorisation is a chain of D dependent column steps; per step: every thread recomputes the pivot (no
// broadcast barrier), rows scale their column entry, ONE barrier, the trailing update spread over 256 threads,
// ONE barrier.  The diagonal goes to a side array so nobody reads a value another thread is replacing.
__global__ void __launch_bounds__(256) k_fit(SampleArgs a, int NBLK) {
    PROMP_SMEM_DECL;
    const int D = a.D, DA = D + 1;
    double* G = (double*)PROMP_SMEM_PTR;
    double* Wm = G + DA * DA;
    double* yv = Wm + DA * DA;
    double* wv = yv + DA;
    double* dg = wv + DA;
    int* flag = (int*)(dg + DA);
    const int tid = threadIdx.x, task = blockIdx.x;
    const int NPAIR = NBLK * (NBLK + 1) / 2;
    // 1. sum the task's partial Gram blocks in workgroup order and scatter into the symmetric matrix
    const int wg0 = a.task_wg_offsets[task], wg1 = a.task_wg_offsets[task + 1];
    for (int e = tid; e < NPAIR * 256; e += 256) {
        double s = 0.0;
#pragma unroll 4
        for (int wg = wg0; wg < wg1; ++wg) s += a.gram_partials[(long long)wg * (NPAIR * 256) + e];
        gram_scatter_entry(s, e, NBLK, D, G);
    }
    __syncthreads();
    // 2. Cholesky of (G[:D,:D] + reg I) carrying the right-hand-side row D along (forward solve for free),
    //    then back substitution; NaN => reg *= 10, at most 5 tries (linear_baseline.py:68-77)
    const float rDA = 1.0f / (float)DA;
    double reg = a.reg;
    for (int attempt = 0; attempt < 5; ++attempt) {
        for (int e = tid; e < DA * DA; e += 256) {
            const int i = (int)(((float)e + 0.5f) * rDA), j = e - i * DA;
            Wm[e] = G[e] + ((i == j && i < D) ? reg : 0.0);
        }
        __syncthreads();
        for (int j = 0; j < D; ++j) {
            const double piv = sqrt(Wm[j * DA + j]);
            if (tid > j && tid <= D) Wm[tid * DA + j] /= piv;
            if (tid == j) dg[j] = piv;
            __syncthreads();
            const int nr = D - j, nc = D - j - 1;  // rows j+1..D, cols j+1..D-1
            const float rnc = 1.0f / (float)(nc > 0 ? nc : 1);
            for (int e = tid; e < nr * nc; e += 256) {
                const int io = (int)(((float)e + 0.5f) * rnc);
                const int i = j + 1 + io, k = j + 1 + (e - io * nc);
                if (k <= i) Wm[i * DA + k] -= Wm[i * DA + j] * Wm[k * DA + j];
            }
            __syncthreads();
        }
        if (tid < D) yv[tid] = Wm[D * DA + tid];
        __syncthreads();
        for (int j = D - 1; j >= 0; --j) {
            const double wj = yv[j] / dg[j];
            if (tid == 0) wv[j] = wj;
            if (tid < j) yv[tid] -= Wm[j * DA + tid] * wj;
            __syncthreads();
        }
        if (tid == 0) *flag = 0;
        __syncthreads();
        const int bad = fit_any_nan<true>(wv, D, flag, tid, 256);
        __syncthreads();
        if (!bad) break;
        reg *= 10.0;
    }
    if (tid < D) a.coeffs[(long long)task * a.coeff_stride + tid] = wv[tid];
}

// One column step of k_fit_wave's factorisation (J is a compile-time constant: the steps are instantiated one by one, which
// keeps the row in registers whatever the unroller's size limits say).
template <int J, int DT>
PROMP_DEV void fitw_column(double (&W)[DT], double* colbuf, double* rsv, double& rs, int lane, int D) {
    if (J >= D) return;       // (wave-uniform)
    // pivot and its reciprocal from ONE reciprocal square root (sqrt followed by a division is two long software sequences, this
    // is one); `rs` arrives computed: the previous step started it as soon as column J was final (see below).  Lane J holds the
    // pivot element d, so one multiplication makes its sqrt(d) = d rs there and L[k][J] in the lanes below: no select.
    W[J] *= rs;
    // The finished column also goes to LDS: the columns together are the factor the back substitution reads (no transposition pass).
    colbuf[J * FITWV_CS + lane] = W[J];
    rsv[J] = rs;              // (every lane, the same value: the back substitution reads lane j's reciprocal from here)
    // lane k holds L[k][J] in W[J].  The first trailing column goes alone: it completes column J + 1, whose pivot's reciprocal
    // square root (seed + one correction: five dependent float64 operations) is then issued in pieces BETWEEN the batches of this
    // step's remaining updates (a wave issues in order: the pieces only overlap with independent work that sits between them in
    // the instruction stream; sched_fence pins that order).
    double dn = 1.0, r0 = 1.0, e = 0.0;
    if (J + 1 < DT) {
        W[J + 1] -= W[J] * readlane_f64(W[J], J + 1);
        dn = readlane_f64(W[J + 1], J + 1);
        r0 = rsq_seed(dn);
    }
    // Eight multipliers are read into eight scalar pairs before the first product: a plain loop compiles to "readlane, readlane,
    // s_nop, fma" on ONE pair (41 cycles per column).  What is left is the price of the multipliers themselves: two v_readlane
    // and the product cost 30 cycles per trailing column in any order (990 columns: the 29 k cycles of this phase, measured).
    // Broadcast reads of the LDS copy instead (ds_read2_b64 off one opaque address register, four in flight) were tried and are
    // slower: the LDS round trip sits on every step's dependent path, 34.5 k cycles.
    constexpr int NBATCH = (DT - (J + 2) + 7) / 8;
#pragma unroll
    for (int b = 0; b < (NBATCH > 0 ? NBATCH : 0); ++b) {
        const int k0 = J + 2 + 8 * b;
        double m[8];
        sched_fence();
#pragma unroll
        for (int u = 0; u < 8; ++u) m[u] = (k0 + u < DT) ? readlane_f64(W[J], k0 + u) : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + u < DT) W[k0 + u] -= W[J] * m[u];
        sched_fence();
        if (b == 0) e = rsq_e(dn, r0);
        if (b == 1 || (b == 0 && NBATCH == 1)) rs = rsq_finish(r0, e);
    }
    if (NBATCH <= 0) rs = rsq_finish(r0, rsq_e(dn, r0));
}
template <int DT, int... Js>
PROMP_DEV void fitw_columns(double (&W)[DT], double* colbuf, double* rsv, int lane, int D, std::integer_sequence<int, Js...>) {
    const double d0 = readlane_f64(W[0], 0), s0 = rsq_seed(d0);
    double rs = rsq_finish(s0, rsq_e(d0, s0));
    (fitw_column<Js, DT>(W, colbuf, rsv, rs, lane, D), ...);
}

// k_fit_wave: the same solve as k_fit, one WAVE per task, for D + 1 <= 64 (obs_dim <= 29).
//
// Lane i holds row i of the work matrix in registers (row D = the right-hand side, carried along as in k_fit).  A column
// step of the Cholesky needs the pivot and, per trailing column k, the freshly scaled entry L[k][j] as a wave-uniform
// multiplier: both come out of the owning lane with v_readlane (scalar registers), so a step is
// "readlane, readlane, v_fma_f64" per trailing column with no barrier and no LDS round trip on the dependent chain
// (k_fit: two workgroup barriers plus LDS traffic per column, 49 us at 45 x 45; this: ~12 us).  All lanes update all
// trailing columns (the upper triangle is never read), so there is no per-lane masking either.  The back substitution
// runs over the transposed factor: the rows are written to LDS once and read back by column.
// Same elimination order as k_fit; the column scaling multiplies by 1/sqrt(pivot) instead of dividing by sqrt(pivot), so
// the two kernels agree to rounding (1e-15 relative), not bit for bit.
// DT = compile-time bound on D + 1 (the j / k loops are fully unrolled over it; steps j >= D leave by a uniform branch).
// grid = tasks, block = FITWV_NT: all waves sum the task's partial Gram blocks (many loads in flight), wave 0 factorizes.
#define FITWV_NT 512       // threads of k_fit_wave: eight waves sum the partial blocks, wave 0 factorizes
template <int DT>
__global__ void __launch_bounds__(FITWV_NT) k_fit_wave(SampleArgs a, int NBLK) {
    PROMP_SMEM_DECL;
    SA_STAMPS;
    const int D = a.D, DA = D + 1;
    double* colbuf = (double*)PROMP_SMEM_PTR;     // [DT][FITWV_CS] the factor by columns: column j = lanes' L[lane][j] (fitw_column)
    double* rsv = colbuf + DT * FITWV_CS + 2;     // [64] 1 / L[j][j]
    double* G = colbuf + fitwv_aux(DT);           // [DA][DA] symmetric Gram matrix (kept for the retries)
    const int lane = threadIdx.x & 63, task = blockIdx.x;
    const int NPAIR = NBLK * (NBLK + 1) / 2;
    // 1. sum the task's partial Gram blocks in workgroup order and scatter into the symmetric matrix
    const int wg0 = a.task_wg_offsets[task], wg1 = a.task_wg_offsets[task + 1];
    // Every entry a thread owns (up to five: DA <= 64 means at most ten block pairs) and sixteen partial blocks of each are
    // requested before the first is added (indices past the task's last workgroup read that workgroup again and add nothing):
    // the partial blocks were written by other XCDs a launch ago, a round trip costs ~3 k cycles, and a task has ~14 of them.
    {
        constexpr int NE = 5;
        double sacc[NE];
#pragma unroll
        for (int q = 0; q < NE; ++q) sacc[q] = 0.0;
        for (int base = wg0; base < wg1; base += 16) {
            double v[NE][16];
#pragma unroll
            for (int q = 0; q < NE; ++q) {
                const int e = threadIdx.x + q * FITWV_NT;
                if (e < NPAIR * 256) {
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int wg = base + u < wg1 ? base + u : wg1 - 1;
                        v[q][u] = a.gram_partials[(long long)wg * (NPAIR * 256) + e];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NE; ++q) {
                const int e = threadIdx.x + q * FITWV_NT;
                if (e < NPAIR * 256) {
#pragma unroll
                    for (int u = 0; u < 16; ++u) sacc[q] += (base + u < wg1) ? v[q][u] : 0.0;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const int e = threadIdx.x + q * FITWV_NT;
            if (e < NPAIR * 256) gram_scatter_entry(sacc[q], e, NBLK, D, G);
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    SA_PHASE(0);
    const int row = lane < DA ? lane : DA - 1;    // (lanes >= DA shadow the last row: finite values, never read back)
    double reg = a.reg;
    double wsol = 0.0;
    for (int attempt = 0; attempt < 5; ++attempt) {
        double W[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) W[k] = (k < D) ? G[row * DA + k] + ((k == row) ? reg : 0.0) : 0.0;
        // 2. Cholesky of (G[:D,:D] + reg I) carrying the right-hand-side row D along (forward solve for free)
        fitw_columns<DT>(W, colbuf, rsv, lane, D, std::make_integer_sequence<int, DT>());
        SA_PHASE(1);
        // 3. back substitution over the transposed factor: y[t] -= L[j][t] w[j], j = D-1 .. 0 (lane t holds y[t]).  Lane t's
        // operands L[j][t], j > t, are column t of the factor -- its own slot of the column store, read back into the registers the
        // factorisation has just freed (zeros for j <= t: y[t] then stays what it was when step t used it).  The dependent steps
        // contain no memory access, no select and no division: w[j] = y[j] / L[j][j] is a multiplication by the stored reciprocal.
        wave_fence();
        double y = (lane < D) ? colbuf[lane * FITWV_CS + D] : 0.0;
        const double rdg = rsv[lane < D ? lane : 0];        // lane j: 1 / L[j][j] (the reciprocal square root of its column step)
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            const double l = colbuf[row * FITWV_CS + (k < DA ? k : 0)];
            W[k] = (k < D && row < k) ? l : 0.0;
        }
        SA_PHASE(2);
#pragma unroll
        for (int j = DT - 1; j >= 0; --j) {
            if (j < D) {
                const double wj = readlane_f64(y * rdg, j);
                y -= W[j] * wj;
            }
        }
        wsol = y * rdg;
        wave_sync();
        SA_PHASE(3);
        if (!wave_any(lane < D && wsol != wsol)) break;      // NaN => reg *= 10, at most 5 tries (linear_baseline.py:68-77)
        reg *= 10.0;
    }
    if (lane < D) a.coeffs[(long long)task * a.coeff_stride + lane] = wsol;
#ifdef PROMP_DEV_STAMPS
    if (task == 0 && lane == 0)
        printf("k_fit_wave cycles: partial sums %llu | factorisation %llu | column reads %llu | back substitution %llu\n", ph[0], ph[1], ph[2], ph[3]);
#endif
}

// The task's coefficients into wc (k_gae, k_dice_adjust: the workgroup's dynamic LDS), and one row's prediction b = Phi . w with
// them (LinearBaseline.predict; BASE_ZERO: 0)
PROMP_DEV void baseline_load_coeffs(const SampleArgs& a, int task, int lane, double* wc) {
    if (a.kind != BASE_ZERO)
        for (int i = lane; i < a.D; i += 64) wc[i] = a.coeffs[(long long)task * a.coeff_stride + i];
    __syncthreads();
}
PROMP_DEV double baseline_row(const SampleArgs& a, const double* wc, long long row, int t) {
    const int O = a.O;
    double b = 0.0;
    if (a.kind != BASE_ZERO) {
        int q = 0;
        if (a.kind == BASE_LINFEAT) {
            for (int c = 0; c < O; ++c) {
                double f[2];
                linfeat_obs(a.obs[row * O + c], true, f, 0, 1);
                b += wc[c] * f[0] + wc[O + c] * f[1];
            }
            q = 2 * O;
        }
        const double tau = linfeat_tau(t);
        b += wc[q] * tau + wc[q + 1] * (tau * tau) + wc[q + 2] * (tau * tau * tau) + wc[q + 3];
    }
    return b;
}

// grid = paths, block = 64.  smem: D doubles (the task's coefficients)
__global__ void __launch_bounds__(64) k_gae(SampleArgs a) {
    PROMP_SMEM_DECL;
    double* wc = (double*)PROMP_SMEM_PTR;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.path_row_offsets[p], T = a.path_row_offsets[p + 1] - row0;
    baseline_load_coeffs(a, a.path_task[p], lane, wc);
    const double g = a.gamma, gl = a.gamma * a.lam;
    const double f = pow(gl, (double)(64 - lane));
    double carry = 0.0, bcarry = 0.0, s1 = 0.0, s2 = 0.0, mn = 1e300;
    for (int end = T; end > 0; end -= 64) {
        const int t = end - 64 + lane;
        const bool valid = t >= 0;
        const long long row = (long long)row0 + t;
        const double b = valid ? baseline_row(a, wc, row, t) : 0.0;
        double bn = shfl_down_f64(b, 1);
        if (lane == 63) bn = bcarry;
        const double rw = a.rew64 ? a.rew64[valid ? row : 0] : (double)a.rew[valid ? row : 0];
        const double x = valid ? (rw + g * bn - b) : 0.0;
        double y = suffix_scan_chunk<true>(x, lane, gl);
        y += f * carry;
        if (valid) {
            if (a.bl64 != nullptr) a.bl64[row] = b;
            a.adv64[row] = y;
            s1 += y;
            s2 += y * y;
            mn = y < mn ? y : mn;
        }
        carry = shfl_idx_f64(y, 0);
        bcarry = shfl_idx_f64(b, 0);
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    mn = wave_min_f64(mn);
    if (lane == 0) {
        a.path_mom[3 * p + 0] = s1;
        a.path_mom[3 * p + 1] = s2;
        a.path_mom[3 * p + 2] = mn;
    }
}

// The statistics of a task's values from its paths' moments (path_mom).  pad_length = 0: over the task's rows.  Otherwise over
// the zero-padded [paths, pad_length] array the DiCE sample processor normalises (samplers/dice_sample_processor.py:165-191): the
// zeros add nothing to the sums, count in n, and are the minimum's rival wherever the task has any.
struct TaskStats {
    double mean, sd, mn, scale;   // mn: the raw minimum; scale = rows / n
};
PROMP_DEV TaskStats task_stats(double s1, double s2, double mn, int rows, int paths, int pad_length) {
    double n = (double)rows;
    if (pad_length != 0) {
        n = (double)paths * (double)pad_length;
        if ((long long)rows < (long long)paths * pad_length) mn = mn < 0.0 ? mn : 0.0;
    }
    TaskStats s;
    s.mean = s1 / n;
    double var = s2 / n - s.mean * s.mean;
    var = var > 0.0 ? var : 0.0;
    s.sd = sqrt(var);
    s.mn = mn;
    s.scale = (double)rows / n;
    return s;
}
// what a padded zero becomes (0 where nothing is normalised or shifted); mn: the minimum AFTER normalisation
PROMP_DEV double padded_zero(const TaskStats& s, double mn, int normalize, int positive) {
    double z = 0.0;
    if (normalize) z = (z - s.mean) / (s.sd + 1e-8);
    if (positive) z = (z - mn) + 1e-8;
    return z;
}

// grid = work items, block = 256
__global__ void __launch_bounds__(256) k_normalize(SampleArgs a) {
    __shared__ double st[4];
    const int tid = threadIdx.x;
    const WorkItem wk = a.work[blockIdx.x];
    const int task = wk.task;
    if (tid == 0) {
        double s1 = 0.0, s2 = 0.0, mn = 1e300;
        for (int p = a.task_path_offsets[task]; p < a.task_path_offsets[task + 1]; ++p) {
            s1 += a.path_mom[3 * p];
            s2 += a.path_mom[3 * p + 1];
            mn = a.path_mom[3 * p + 2] < mn ? a.path_mom[3 * p + 2] : mn;
        }
        const int row0 = a.task_row_offsets[task];
        const TaskStats s = task_stats(s1, s2, mn, a.task_row_offsets[task + 1] - row0, a.task_path_offsets[task + 1] - a.task_path_offsets[task],
                                       a.pad_length);
        st[0] = s.mean;
        st[1] = s.sd;
        st[2] = s.mn;
        st[3] = a.pad_scale ? s.scale : 1.0;
        if (a.pad_out != nullptr && wk.row_begin == row0)       // (the task's first work item)
            a.pad_out[task] = padded_zero(s, a.normalize ? (s.mn - s.mean) / (s.sd + 1e-8) : s.mn, a.normalize, a.positive);
    }
    __syncthreads();
    const double mean = st[0], sd = st[1];
    double mn = st[2];
    if (a.normalize) mn = (mn - mean) / (sd + 1e-8);
    for (int row = wk.row_begin + tid; row < wk.row_end; row += 256) {
        double x = a.adv64[row];
        if (a.normalize) x = (x - mean) / (sd + 1e-8);
        if (a.positive) x = (x - mn) + 1e-8;
        if (a.x64 != nullptr) a.x64[row] = x;
        a.adv32[row] = a.pad_scale ? (float)(x * st[3]) : (float)x;
    }
}

// ---------------------------------------------------------------------------------------------
// DiCE sample processing (samplers/dice_sample_processor.py:96-191, utils/utils.py:59-71; float64 restatement:
// oracle/dice.py process_samples_dice): k_dice_targets -> the plan's Gram and fit kernels on that target -> k_dice_adjust ->
// k_dice_finish.  One wave per path, grid = paths, block = 64.
// ---------------------------------------------------------------------------------------------
// y_t = r_t gamma^t into the regression target's place (ret64 / ret32); per path: sum r (path_undisc), sum y (path_ret0: DiCE's
// "discounted return"), sum r^2 (path_rsq).  gamma^t is pow(), not the reference's running product: they differ by rounding.
__global__ void __launch_bounds__(64) k_dice_targets(SampleArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.path_row_offsets[p], T = a.path_row_offsets[p + 1] - row0;
    double usum = 0.0, ysum = 0.0, rsq = 0.0;
    for (int t = lane; t < T; t += 64) {
        const long long row = (long long)row0 + t;
        const double x = a.rew64 ? a.rew64[row] : (double)a.rew[row];
        const double y = x * pow(a.gamma, (double)t);
        a.ret64[row] = y;
        a.ret32[row] = (float)y;
        usum += x;
        ysum += y;
        rsq += x * x;
    }
    usum = wave_sum_f64(usum);
    ysum = wave_sum_f64(ysum);
    rsq = wave_sum_f64(rsq);
    if (lane == 0) {
        a.path_undisc[p] = usum;
        a.path_ret0[p] = ysum;
        a.path_rsq[p] = rsq;
    }
}

// adj = y - Phi . w into adv64, its moments into path_mom.  smem: D doubles (the task's coefficients), as k_gae
__global__ void __launch_bounds__(64) k_dice_adjust(SampleArgs a) {
    PROMP_SMEM_DECL;
    double* wc = (double*)PROMP_SMEM_PTR;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.path_row_offsets[p], T = a.path_row_offsets[p + 1] - row0;
    baseline_load_coeffs(a, a.path_task[p], lane, wc);
    double s1 = 0.0, s2 = 0.0, mn = 1e300;
    for (int t = lane; t < T; t += 64) {
        const long long row = (long long)row0 + t;
        const double adj = a.ret64[row] - baseline_row(a, wc, row, t);
        a.adv64[row] = adj;
        s1 += adj;
        s2 += adj * adj;
        mn = adj < mn ? adj : mn;
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    mn = wave_min_f64(mn);
    if (lane == 0) {
        a.path_mom[3 * p + 0] = s1;
        a.path_mom[3 * p + 1] = s2;
        a.path_mom[3 * p + 2] = mn;
    }
}

// The adjusted rewards normalised / shifted over the task's padded array (x64), the rewards of the DiCE objective
// dice_rw = float(x rows / n), their suffix sums within the path (adv32: the gradient weights, k_dice_scan's mode 0) and the
// task's pad value.  Every wave of a task sums the task's path moments itself, lane by lane in path order and then across the
// wave: the same order whatever the grid.
__global__ void __launch_bounds__(64) k_dice_finish(SampleArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.path_row_offsets[p], T = a.path_row_offsets[p + 1] - row0;
    const int task = a.path_task[p];
    const int p0 = a.task_path_offsets[task], p1 = a.task_path_offsets[task + 1];
    double s1 = 0.0, s2 = 0.0, mn = 1e300;
    for (int q = p0 + lane; q < p1; q += 64) {
        s1 += a.path_mom[3 * q];
        s2 += a.path_mom[3 * q + 1];
        mn = a.path_mom[3 * q + 2] < mn ? a.path_mom[3 * q + 2] : mn;
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    mn = wave_min_f64(mn);
    const TaskStats s = task_stats(s1, s2, mn, a.task_row_offsets[task + 1] - a.task_row_offsets[task], p1 - p0, a.pad_length);
    const double mean = s.mean, sd = s.sd;
    mn = s.mn;
    if (a.normalize) mn = (mn - mean) / (sd + 1e-8);
    if (p == p0 && lane == 0) a.pad_out[task] = padded_zero(s, mn, a.normalize, a.positive);
    double carry = 0.0;
    for (int end = T; end > 0; end -= 64) {
        const int t = end - 64 + lane;
        const long long row = (long long)row0 + t;
        double w = 0.0;
        if (t >= 0) {
            double x = a.adv64[row];
            if (a.normalize) x = (x - mean) / (sd + 1e-8);
            if (a.positive) x = (x - mn) + 1e-8;
            a.x64[row] = x;
            const float rw = (float)(x * s.scale);
            a.dice_rw[row] = rw;
            w = (double)rw;
        }
        const double y = suffix_scan_chunk<false>(w, lane) + carry;
        if (t >= 0) a.adv32[row] = (float)y;
        carry = shfl_idx_f64(y, 0);
    }
}

// ---------------------------------------------------------------------------------------------
// Wide observations (obs_dim > 32, i.e. more than 68 features: Ant's 2*111 + 4 = 226).  k_gram<NBLK> stages raw
// observation rows of at most 32 floats per wave and k_fit keeps two (D+1)^2 matrices in LDS; beyond that:
//
// k_gram_wide: the upper-triangular 16x16 block pairs of [Phi R]^T [Phi R] no longer fit one wave's registers
// (120 pairs at D = 226), so the workgroup shares the feature tile: 8 waves, wave w owns a contiguous eighth of the pair list
// (<= GRAMW_PPW of them) over ALL rows of the work item -- no cross-wave reduction, each partial block is written by
// its owner.  Rounds of GRAMW_ROWS rows; out: the partial layout above.
// grid = work items (table 0) x pair slices, block = 512.  smem: the feature tile, ROWS * FS doubles.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512, 2) k_gram_wide(SampleArgs a, int NBLK, int GRAMW_ROWS) {
    PROMP_SMEM_DECL;
    const int tid = threadIdx.x, lane = tid & 63, w = wave_uniform(tid >> 6), i16 = lane & 15, kk = lane >> 4;
    const int FS = gramw_fs(NBLK), NPAIR = NBLK * (NBLK + 1) / 2, NC = 16 * NBLK;
    double* Phi = (double*)PROMP_SMEM_PTR;
    const WorkItem wk = a.work[blockIdx.x];
    const int O = a.O, D = a.D;
    // this wave's pairs: a contiguous range of the row-major list (bi, bj >= bi); offsets of the two 16-column blocks inside a
    // feature row (wave-uniform)
    // (gridDim.y > 1: this workgroup's slice of the list first)
    const int npy = (NPAIR + (int)gridDim.y - 1) / (int)gridDim.y, py0 = npy * (int)blockIdx.y;
    const int pend = py0 + npy < NPAIR ? py0 + npy : NPAIR;
    const int ppw = (npy + 7) / 8, p0 = py0 + w * ppw;
    int ca[GRAMW_PPW], cb[GRAMW_PPW];
#pragma unroll
    for (int j = 0; j < GRAMW_PPW; ++j) {
        const int p = p0 + j;
        int bi, bj;
        tri_pair_blocks((j < ppw && p < pend) ? p : 0, NBLK, bi, bj);
        ca[j] = 16 * bi;
        cb[j] = 16 * bj;
    }
    f64x4 acc[GRAMW_PPW];
#pragma unroll
    for (int j = 0; j < GRAMW_PPW; ++j) acc[j] = zero4d();
    // The feature tile is written straight from the loaded observations (element e of the [ROWS][O] chunk is observation e mod O
    // of row e / O: columns c and O + c), 16 loads per thread in flight; threads 0 .. ROWS - 1 add their row's time features, the
    // constant and the target.  Columns past D + 1 are zeroed once.  (Until round 4 the rows were staged raw in LDS and every
    // feature column went through a branch tree: k_gram's 32.8 k of 52 k cycles.)
    for (int e = tid; e < GRAMW_ROWS * FS; e += 512) Phi[e] = 0.0;
    const float rO = 1.0f / (float)(O > 0 ? O : 1);
    const int qt = (a.kind == BASE_LINFEAT) ? 2 * O : 0;        // first of the four time columns (tau, tau^2, tau^3, 1)
    for (int base = wk.row_begin; base < wk.row_end; base += GRAMW_ROWS) {
        const int nrows = (wk.row_end - base) < GRAMW_ROWS ? (wk.row_end - base) : GRAMW_ROWS;
        __syncthreads();   // the previous round's MFMAs are done with Phi (first round: the zeros are in place)
        if (a.kind == BASE_LINFEAT) {
            const int lim = nrows * O, tot = GRAMW_ROWS * O;
            for (int e0 = tid; e0 < tot; e0 += 512 * 16) {
                float x[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int e = e0 + 512 * u;
                    x[u] = a.obs[(long long)base * O + (e < lim ? e : 0)];
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int e = e0 + 512 * u;
                    if (e < tot) {
                        const int r = (int)(((float)e + 0.5f) * rO), c = e - r * O;
                        linfeat_obs(x[u], e < lim, Phi, r * FS + c, r * FS + O + c);
                    }
                }
            }
        }
        if (tid < GRAMW_ROWS) {
            const bool rv = tid < nrows;
            const int r = rv ? tid : 0;
            linfeat_row_tail(Phi + tid * FS, qt, D, rv, a.row_t[base + r], a.ret64[base + r]);
        }
        __syncthreads();
        // The products, software-pipelined: the operands of the NEXT group of four pairs are requested before the current group's
        // four matrix instructions issue (4 x 64 cycles of FP64 MFMA cover the LDS round trip).  Loading a group, waiting, then
        // issuing its products left the matrix pipe idle two thirds of the time (PMC: SQ_VALU_MFMA_BUSY_CYCLES 33 % of the
        // kernel, SQ_WAIT_ANY 50 % of the wave cycles).  Pairs beyond the wave's share read a valid address and are not issued.
        {
            constexpr int NG = GRAMW_PPW / 4;
            const int nsteps = GRAMW_ROWS / 4;
            double xa[4], xb[4];
            const double* row = Phi + kk * FS + i16;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xa[u] = row[ca[u]];
                xb[u] = row[cb[u]];
            }
#pragma unroll 1
            for (int st = 0; st < nsteps; ++st) {
                const double* rnext = Phi + (4 * (st + 1 < nsteps ? st + 1 : st) + kk) * FS + i16;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    double na[4], nb[4];
                    const double* src = (g + 1 < NG) ? row : rnext;
                    const int gn = (g + 1 < NG) ? g + 1 : 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        na[u] = src[ca[4 * gn + u]];
                        nb[u] = src[cb[4 * gn + u]];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = 4 * g + u;
                        if (j < ppw && p0 + j < pend) acc[j] = mfma16d(xa[u], xb[u], acc[j]);      // (wave-uniform)
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        xa[u] = na[u];
                        xb[u] = nb[u];
                    }
                    sched_fence();
                }
                row = rnext;
            }
        }
    }
    double* out = a.gram_partials + (long long)blockIdx.x * (NPAIR * 256);
#pragma unroll
    for (int j = 0; j < GRAMW_PPW; ++j) {
        const int p = p0 + j;
        if (j < ppw && p < pend) gram_store_block(out, p, acc[j], kk, i16);
    }
}

// ---------------------------------------------------------------------------------------------
// k_gram_tiled (round 5, second half): the same product as k_gram_wide with the operands of the FP64 matrix instruction REUSED in
// registers.  k_gram_wide reads two LDS operands per v_mfma_f64_16x16x4_f64 (its waves own arbitrary runs of the pair list, so the
// shared row block of a run is fetched again for every pair): 40 ds_read_b64 per 15 products and wave at Ant's width, two thirds
// of the LDS bandwidth of the CU when the matrix pipe is full -- the pipe measured 44 % busy.  Here a wave owns a SQUARE of
// TB x TB column blocks (bands of TB = 3 blocks, 48 feature columns; band pair bi <= bj): 3 + 3 operand reads feed 9 products, at
// immediate offsets from two lane addresses.  Squares on the diagonal issue their upper triangle (6 products from 3 reads).  The
// two shapes are two instances of the step loop: products behind wave-uniform branches, or more loop shapes (short last bands),
// made the register allocator spill accumulators -- the block count is padded to whole bands instead (the padding columns are
// zero in the tile and are never written out).  out[] is the partial layout above, whichever Gram kernel wrote
// it: k_gram_sum_wide / the fits do not change.
//   * Ant's 15 blocks are 5 bands = 15 squares = 15 waves of ONE workgroup (10 x 9 + 5 x 6 = 120 products per k-step, the
//     unpadded count); the host shares them out over the SIMDs by cost (GramtMap; wave w runs on SIMD w mod 4).  More squares:
//     slices of NWV along gridDim.y (Humanoid's 48 blocks: 136 squares, 9 slices).
//   * The feature tile is double-buffered where two tiles fit LDS (Ant: 2 x 32 rows x 240 columns = 123 KB): the observations
//     of round r + 1 are requested before the products of round r and written into the other tile behind them -- one barrier
//     per round, the global latency and the tile build off the matrix pipe's path.  Wider tiles (Humanoid: 16 rows x 784) are
//     single: the request is still issued a round ahead, the write sits between two barriers.
//   * A partial last round issues only the k-steps that hold rows.
// grid = work items (table 0) x slices, block = 64 NWV.  ROWS / DB: gramt_cfg; smem: gramt_smem(NBLK, ROWS, DB).
// ---------------------------------------------------------------------------------------------
PROMP_HD size_t gramt_smem(int NBLK, int rows, int db) { return sizeof(double) * (size_t)((db ? 2 : 1) * rows * gramt_fs(NBLK)); }

// which of a square's TB x TB products a wave of shape SHAPE issues: all (off the diagonal); the upper triangle jj >= ii (a
// diagonal square); the triangle's first row / its other rows (a diagonal square shared by two waves: with a wave to spare the
// host splits one so that the four SIMDs carry the same number of products)
template <int SHAPE>
PROMP_HD PROMP_CX bool gramt_has(int ii, int jj) {
    return SHAPE == GRAMT_FULL ? true : SHAPE == GRAMT_DIAG ? jj >= ii : SHAPE == GRAMT_DIAG_TOP ? ii == 0 : (ii >= 1 && jj >= ii);
}
// the k-steps of one round for one square: pa / pb = this lane's element of the first block of the row / column band in k-row
// kk of the tile; FS4 = 4 rows of the tile.  On the diagonal the column band IS the row band: one set of operands.
template <int TB, int SHAPE>
PROMP_DEV void gramt_steps(f64x4 (&acc)[TB][TB], const double* pa, const double* pb, int nst, int FS4) {
    constexpr bool DIAG = SHAPE != GRAMT_FULL;
#pragma unroll 1
    for (int st = 0; st < nst; ++st) {
        double fa[TB], fb[TB];
#pragma unroll
        for (int u = 0; u < TB; ++u) {
            fa[u] = pa[16 * u];
            fb[u] = DIAG ? fa[u] : pb[16 * u];
        }
#pragma unroll
        for (int ii = 0; ii < TB; ++ii)
#pragma unroll
            for (int jj = 0; jj < TB; ++jj)
                if (gramt_has<SHAPE>(ii, jj)) acc[ii][jj] = mfma16d(fa[ii], fb[jj], acc[ii][jj]);
        pa += FS4;
        pb += FS4;
    }
}

// One wave's whole walk over the work item's rows for its square (bi, bj); SHAPE: GRAMT_*.  The shapes are separate instances of
// the WHOLE walk, accumulators included: with one set of accumulators around two step loops the compiler gave each loop its own
// registers for them (72 + 48 of 128) and spilled.  Every wave passes the same barriers whatever its shape.
template <int TB, int NWV, int NLD, int SHAPE>
PROMP_DEV void gramt_walk(const SampleArgs& a, int NBLK, int ROWS, int DB, double* Phi, bool active, int bi, int bj) {
    constexpr int NT = 64 * NWV;
    const int tid = threadIdx.x, lane = tid & 63, i16 = lane & 15, kk = lane >> 4;
    const int FS = gramt_fs(NBLK);
    const int O = a.O, D = a.D;
    const WorkItem wk = a.work[blockIdx.x];
    f64x4 acc[TB][TB];
#pragma unroll
    for (int ii = 0; ii < TB; ++ii)
#pragma unroll
        for (int jj = 0; jj < TB; ++jj) acc[ii][jj] = zero4d();

    // The tile build: element e of the round's [ROWS][O] chunk of observations is observation e mod O of row
    // e / O and goes to columns c and O + c; threads 0 .. ROWS - 1 add their row's time features, the constant and the target.
    // Split in two: the requests (into x[], tgt, rt) and, a round of products later, the writes.
    const float rO = 1.0f / (float)(O > 0 ? O : 1);
    const int qt = (a.kind == BASE_LINFEAT) ? 2 * O : 0;        // first of the four time columns (tau, tau^2, tau^3, 1)
    const int tot = ROWS * O;
    float x[NLD];
    double tgt = 0.0;
    int rt = 0;
    auto request = [&](int base, int nrows) {
        if (a.kind == BASE_LINFEAT) {
            const int lim = nrows * O;
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int e = tid + NT * u;
                x[u] = a.obs[(long long)base * O + (e < lim ? e : 0)];
            }
        }
        if (tid < ROWS) {
            const int r = tid < nrows ? tid : 0;
            tgt = a.ret64[base + r];
            rt = a.row_t[base + r];
        }
    };
    auto build = [&](double* buf, int nrows) {
        if (a.kind == BASE_LINFEAT) {
            const int lim = nrows * O;
            // (the positions are recomputed every round: kept across the products they would cost 2 NLD registers)
            const int oz = opaque_zero();
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int e = tid + NT * u + oz;
                if (e < tot) {
                    const int r = (int)(((float)e + 0.5f) * rO), c = e - r * O;
                    linfeat_obs(x[u], e < lim, buf, r * FS + c, r * FS + O + c);
                }
                sched_fence();      // one element at a time: interleaved, the NLD elements' temporaries push accumulators into scratch
            }
        }
        if (tid < ROWS) linfeat_row_tail(buf + tid * FS, qt, D, tid < nrows, rt, tgt);
    };

    for (int e = tid; e < (DB ? 2 : 1) * ROWS * FS; e += NT) Phi[e] = 0.0;      // columns past D + 1 stay zero
    __syncthreads();
    {
        const int n0 = (wk.row_end - wk.row_begin) < ROWS ? (wk.row_end - wk.row_begin) : ROWS;
        request(wk.row_begin, n0);
        build(Phi, n0);
    }
    __syncthreads();
    int cur = 0;
    const int lofs = kk * FS + i16;
    for (int base = wk.row_begin; base < wk.row_end; base += ROWS) {
        const int nrows = (wk.row_end - base) < ROWS ? (wk.row_end - base) : ROWS;
        const int nbase = base + ROWS;
        const bool more = nbase < wk.row_end;
        const int nnext = (wk.row_end - nbase) < ROWS ? (wk.row_end - nbase) : ROWS;
        if (more) request(nbase, nnext);
        const double* buf = Phi + cur * ROWS * FS;
        if (active) {
            const int nst = (nrows + 3) >> 2;
            const double* pa = buf + lofs + 16 * TB * bi;
            const double* pb = buf + lofs + 16 * TB * bj;
            gramt_steps<TB, SHAPE>(acc, pa, pb, nst, 4 * FS);
        }
        if (DB) {
            if (more) build(Phi + (cur ^ 1) * ROWS * FS, nnext);    // nobody reads that tile before the barrier below
            __syncthreads();
            cur ^= 1;
        } else {
            __syncthreads();                                        // the products of this round are done with the tile
            if (more) build(Phi, nnext);
            __syncthreads();
        }
    }
    const int NPAIR = NBLK * (NBLK + 1) / 2;
    double* out = a.gram_partials + (long long)blockIdx.x * (NPAIR * 256);
#pragma unroll
    for (int ii = 0; ii < TB; ++ii)
#pragma unroll
        for (int jj = 0; jj < TB; ++jj) {
            const int gi = TB * bi + ii, gj = TB * bj + jj;
            if (active && gramt_has<SHAPE>(ii, jj) && gj < NBLK) gram_store_block(out, tri_pair_index(gi, gj, NBLK), acc[ii][jj], kk, i16);
        }
}

template <int TB, int NWV, int NLD>
__global__ void __launch_bounds__(64 * NWV) k_gram_tiled(SampleArgs a, int NBLK, GramtMap map, int ROWS, int DB) {
    PROMP_SMEM_DECL;
    const int w = wave_uniform((int)threadIdx.x >> 6);
    const int NB = gramt_nb(NBLK), NR = NB * (NB + 1) / 2;
    // this wave's square: band pair bi <= bj of the row-major list
    const int rect = wave_uniform(gridDim.y == 1 ? (int)map.rect[w] : (int)blockIdx.y * NWV + w);
    const bool active = rect < NR;
    int bi, bj;
    tri_pair_blocks(active ? rect : 0, NB, bi, bj);
    const int part = wave_uniform(gridDim.y == 1 ? (int)map.part[w] : GRAMT_DIAG);
    double* Phi = (double*)PROMP_SMEM_PTR;
    if (bi != bj) gramt_walk<TB, NWV, NLD, GRAMT_FULL>(a, NBLK, ROWS, DB, Phi, active, bi, bj);
    else if (part == GRAMT_DIAG_TOP) gramt_walk<TB, NWV, NLD, GRAMT_DIAG_TOP>(a, NBLK, ROWS, DB, Phi, active, bi, bj);
    else if (part == GRAMT_DIAG_REST) gramt_walk<TB, NWV, NLD, GRAMT_DIAG_REST>(a, NBLK, ROWS, DB, Phi, active, bi, bj);
    else gramt_walk<TB, NWV, NLD, GRAMT_DIAG>(a, NBLK, ROWS, DB, Phi, active, bi, bj);
}

// ---------------------------------------------------------------------------------------------
// k_fit_wide: the same solve as k_fit when the (D+1)^2 matrices do not fit in LDS (Ant: D = 226).  G and the work matrix live in
// global memory (L2-resident, 0.4 MB per task).  Right-looking blocked Cholesky, 32-column panels through LDS, the right-hand
// side carried along as row D (k_fit's forward solve for free):
// the panel's diagonal block in one wave's registers (chol_diag_block), the rows below it one per thread (chol_rows_below), the
// rank-32 update of the trailing matrix on the FP64 matrix cores, all waves (chol_trailing_update).
// The back substitution walks the factor in 32-row blocks: one wave solves the block's triangle in registers, all threads apply
// its 32 solved entries to the rows above.  Round 3's version took two workgroup barriers per COLUMN (226 x 2, plus 226 in the
// back substitution) and updated the trailing matrix with scalar FMAs: 676 us per launch at Ant's size; this one takes four
// barriers per PANEL.  Same elimination order and arithmetic as k_fit up to the reciprocal square root k_fit_wave also uses
// (results agree to rounding, not bit for bit).
// grid = tasks, block = FITW_NT.  smem: fitw_smem(D).
// ---------------------------------------------------------------------------------------------
// The task's partial Gram blocks summed in workgroup order and scattered into the symmetric matrix G -- and G + reg I into the
// work matrix of the first factorisation attempt -- by the WHOLE chip (grid = tasks x fitw_sum_split(NBLK)): inside k_fit_wide the sum
// ran on one compute unit per task (40 of 256 busy, a quarter of that kernel's time at Ant's size).
// scratch: [tasks][2][(D+1)^2].  block = 256.
// (the split grows with the matrix: Humanoid's 1176 blocks of 256 entries per task are 617 MB of partial blocks per launch, and with
//  8 workgroups per task the loads in flight -- not the memory system -- set the pace; every entry is still one thread's sum in workgroup order)
__global__ void __launch_bounds__(256) k_gram_sum_wide(SampleArgs a, int NBLK, double* scratch, int FITW_SUM_SPLIT) {
    const int D = a.D, DA = D + 1;
    const int task = blockIdx.x / FITW_SUM_SPLIT, part = blockIdx.x % FITW_SUM_SPLIT;
    double* G = scratch + (size_t)task * 2 * DA * DA;
    double* Wm = G + (size_t)DA * DA;
    const int NPAIR = NBLK * (NBLK + 1) / 2;
    const int wg0 = a.task_wg_offsets[task], wg1 = a.task_wg_offsets[task + 1];
    for (int e = part * 256 + threadIdx.x; e < NPAIR * 256; e += 256 * FITW_SUM_SPLIT) {
        // eight partial blocks per trip, all requested before the first is added (as k_fit_wave)
        double s = 0.0;
        for (int base = wg0; base < wg1; base += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int wg = base + u < wg1 ? base + u : wg1 - 1;
                v[u] = a.gram_partials[(long long)wg * (NPAIR * 256) + e];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (base + u < wg1) ? v[u] : 0.0;
        }
        gram_scatter_entry<true>(s, e, NBLK, D, G, Wm, a.reg);
    }
}

// Back substitution L^T w = z over the factor's NB-row blocks from the bottom up (k_fit_wide, k_fitw_back): wave 0 solves the block's
// triangle in registers (lane t holds y[kb + t] and column t of the transposed triangle), the other waves then apply the block's
// solved entries to the rows above, one row per thread.  yv = z on entry (LDS, written by the caller without a barrier), rdv =
// 1 / diag(L) (LDS, likewise), the result goes to wv (LDS); tri: 2 x NB x (NB + 1) doubles of LDS.
// The factor lives in global memory (L2) and is final, so nothing taken from there depends on the solve: a thread requests the NB
// factor entries of its row BEFORE wave 0 solves the block, and the NEXT block's triangle is requested at the same point (by waves
// 1.., a few entries per thread, parked in LDS behind the first barrier: in wave 0's registers a second triangle spilled) -- a block
// costs one solve (NB dependent steps) instead of two round trips to L2 plus the solve (21 % of k_fit_wide's time at Ant's 8 blocks;
// 48 blocks at Humanoid's width).  Same operations on the same values in the same order as the loop it replaces.
template <int NB>
PROMP_DEV void fitw_back_substitute(const double* Wm, int D, int DA, double* yv, double* wv, const double* rdv, double* tri, int tid,
                                    int lane, int w) {
    constexpr int NT = FITW_NT, NH = NT - 64, TS = NB + 1, NTV = (NB * NB + NH - 1) / NH;
    const int row = tid - 64;                 // (wave 0 solves; the rows above and the prefetch belong to the other waves)
    int kb = ((D - 1) / NB) * NB, cur = 0;
    {
        const int nb = (D - kb) < NB ? (D - kb) : NB;
        for (int e = row; e >= 0 && e < NB * NB; e += NH) {
            const int j = e / NB, t = e - j * NB;
            if (j < nb && j > t) tri[j * TS + t] = Wm[(size_t)(kb + j) * DA + kb + t];
        }
    }
    __syncthreads();
    for (; kb >= 0; kb -= NB) {
        const int nb = (D - kb) < NB ? (D - kb) : NB;
        const bool mine = row >= 0 && row < kb;
        double lv[NB], tv[NTV];
        if (mine) {
#pragma unroll
            for (int r = 0; r < NB; ++r) lv[r] = Wm[(size_t)(kb + (r < nb ? r : 0)) * DA + row];     // all in flight together
        }
        if (row >= 0 && kb >= NB) {           // the next block's triangle (every block above the last one is full)
            const int kn = kb - NB;
#pragma unroll
            for (int u = 0; u < NTV; ++u) {
                const int e = row + u * NH, j = e / NB, t = e - j * NB;
                tv[u] = (e < NB * NB && j > t) ? Wm[(size_t)(kn + j) * DA + kn + t] : 0.0;
            }
        }
        if (w == 0) {
            const int t = lane < nb ? lane : nb - 1;
            const double* T = tri + cur * NB * TS;
            double W[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) W[j] = (j < nb && j > t) ? T[j * TS + t] : 0.0;
            double y = yv[kb + t];
            const double rd = rdv[kb + t];
            double wsol = 0.0;
#pragma unroll
            for (int j = NB - 1; j >= 0; --j) {
                if (j < nb) {
                    const double wj = readlane_f64(y, j) * readlane_f64(rd, j);
                    if (lane == j) wsol = wj;
                    if (lane < j) y -= W[j] * wj;
                }
            }
            if (lane < nb) wv[kb + lane] = wsol;
        }
        __syncthreads();
        // the rows above: y[i] -= sum_r L[kb + r][i] w[kb + r]
        if (mine) {
            double s = yv[row];
#pragma unroll
            for (int r = 0; r < NB; ++r) s -= (r < nb) ? lv[r] * wv[kb + r] : 0.0;
            yv[row] = s;
        }
        for (int i = row + NH; row >= 0 && i < kb; i += NH) {         // (more than NT - 64 rows above: Humanoid's first blocks)
            double l2[NB];
#pragma unroll
            for (int r = 0; r < NB; ++r) l2[r] = Wm[(size_t)(kb + (r < nb ? r : 0)) * DA + i];
            double s = yv[i];
#pragma unroll
            for (int r = 0; r < NB; ++r) s -= (r < nb) ? l2[r] * wv[kb + r] : 0.0;
            yv[i] = s;
        }
        if (row >= 0 && kb >= NB) {
            double* Tn = tri + (cur ^ 1) * NB * TS;
#pragma unroll
            for (int u = 0; u < NTV; ++u) {
                const int e = row + u * NH, j = e / NB, t = e - j * NB;
                if (e < NB * NB && j > t) Tn[j * TS + t] = tv[u];
            }
        }
        cur ^= 1;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// The steps of one NB-column panel of the blocked right-looking Cholesky (k_fit_wide runs them in one workgroup per task,
// k_fitw_panel / k_fitw_update one launch per phase: the same functions, so the two agree bit for bit).  The panel sits in LDS
// as Pn[row][NB + 1]; Wm is the task's (D + 1) x (D + 1) work matrix in global memory, row D the right-hand side; nb <= NB the
// panel's columns (a last panel may be narrower).  Barriers between the steps are the caller's.
// ---------------------------------------------------------------------------------------------
// rows row0 .. row0 + nrows - 1, columns col0 .. col0 + nb - 1 of Wm into Pn, the columns past nb and PAD more rows as zeros
// (the trailing update reads whole 16-row tiles)
template <int NB>
PROMP_CX int chol_log_nb() { return NB == 32 ? 5 : 4; }       // (panels are 32 or 16 columns wide)
template <int NB, int PAD>
PROMP_DEV void chol_panel_load(double* Pn, const double* Wm, int DA, int row0, int col0, int nrows, int nb, int tid) {
    constexpr int PS = NB + 1, LOG_NB = chol_log_nb<NB>();
    for (int e = tid; e < (nrows + PAD) * NB; e += FITW_NT) {
        const int i = e >> LOG_NB, c = e & (NB - 1);
        Pn[i * PS + c] = (c < nb && (PAD == 0 || i < nrows)) ? Wm[(size_t)(row0 + i) * DA + col0 + c] : 0.0;
    }
}
// The panel's NB x NB diagonal block, factorised by ONE wave in registers: a row per lane (lanes >= nb shadow the last row:
// finite, never stored), pivots and multipliers by v_readlane -- nb dependent steps with no barrier and no memory access on the
// chain.  Leaves L (diagonal included) in Pn, 1 / L[c][c] in rdp[c] and, KEEP_DIAG, L[c][c] in dg[c].
template <int NB, bool KEEP_DIAG>
PROMP_DEV void chol_diag_block(double* Pn, double* rdp, double* dg, int nb, int lane) {
    constexpr int PS = NB + 1;
    const int row = lane < nb ? lane : nb - 1;
    double W[NB];
    double rdg = 1.0, dgv = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) W[k] = Pn[row * PS + k];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j < nb) {     // (wave-uniform)
            const double dj = readlane_f64(W[j], j), rs = rsqrt(dj), piv = dj * rs;
            W[j] = (lane == j) ? piv : W[j] * rs;
            rdg = (lane == j) ? rs : rdg;
            dgv = (lane == j) ? piv : dgv;       // (W[lane] read at the end would index the array by a runtime value: the
                                                 //  whole row then lives in scratch memory, loop included)
#pragma unroll
            for (int k = j + 1; k < NB; ++k) W[k] -= W[j] * readlane_f64(W[j], k);     // lane k holds L[k][j] in W[j]
        }
    }
    if (lane < nb) {
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if (k <= lane) Pn[lane * PS + k] = W[k];
        if (KEEP_DIAG) dg[lane] = dgv;
        rdp[lane] = rdg;
    }
}
// The nbelow rows under the diagonal block (the right-hand side among them): x L^T = a, one row per thread, forward
// substitution over the block's columns.
template <int NB>
PROMP_DEV void chol_rows_below(double* Pn, const double* rdp, int nb, int nbelow, int tid) {
    constexpr int PS = NB + 1;
    for (int rr = tid; rr < nbelow; rr += FITW_NT) {       // (one trip up to 512 rows below the block)
        double* xr = Pn + (size_t)(nb + rr) * PS;
        double x[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) x[c] = xr[c];
        // column by column, right-looking: once x[c] is final the later entries take their x[c] L[c2][c] at once -- NB - 1 - c
        // independent multiply-adds (the left-looking form is one dependent chain of c per entry).  L[c2][c] is the same
        // address in every lane: a broadcast.  In a last panel narrower than NB the rows / columns >= nb of the block hold
        // other rows' data: finite junk that only reaches entries >= nb, which are stored as 0.
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if (c < nb) {
                x[c] *= rdp[c];
#pragma unroll
                for (int c2 = c + 1; c2 < NB; ++c2) x[c2] -= x[c] * Pn[c2 * PS + c];
            }
        }
#pragma unroll
        for (int c = 0; c < NB; ++c) xr[c] = (c < nb) ? x[c] : 0.0;
    }
}
// the factored panel (nr rows from the diagonal block's first) back into Wm: the part below the diagonal and the right-hand-side
// row; with_diag: the diagonal too
template <int NB>
PROMP_DEV void chol_panel_store(double* Wm, const double* Pn, int DA, int k0, int nr, int nb, bool with_diag, int tid) {
    constexpr int PS = NB + 1, LOG_NB = chol_log_nb<NB>();
    for (int e = tid; e < nr * NB; e += FITW_NT) {
        const int i = e >> LOG_NB, c = e & (NB - 1);
        if (c < nb && (with_diag ? i >= c : i > c)) Wm[(size_t)(k0 + i) * DA + k0 + c] = Pn[i * PS + c];
    }
}
// Rank-nb update of the trailing matrix on the FP64 matrix cores: rows k1..D, columns k1..D-1 of Wm -= panel panel^T over the
// 16 x 16 tiles of the lower triangle; this wave takes tiles first, first + stride, ...  The panel's rows below its diagonal
// block start at row prow0 of Pn and are followed by 16 rows of zeros.  Every trailing entry takes one NB-term MFMA sum
// whichever wave computes it.
template <int NB>
PROMP_DEV void chol_trailing_update(double* Wm, const double* Pn, int prow0, int D, int k1, int first, int stride, int lane) {
    constexpr int PS = NB + 1;
    const int DA = D + 1, i16 = lane & 15, kk = lane >> 4;
    const int tr = DA - k1, tc = D - k1;
    const int nti = (tr + 15) >> 4, ntj = (tc + 15) >> 4;
    const int ntile = nti * ntj;                    // (tiles above the diagonal are skipped below)
    for (int tix = first; tix < ntile; tix += stride) {
        const int bi = tix / ntj, bj = tix - bi * ntj;
        if (bj > bi) continue;                     // wave-uniform
        const double* pa = Pn + (size_t)(prow0 + 16 * bi + i16) * PS + kk;
        const double* pb = Pn + (size_t)(prow0 + 16 * bj + i16) * PS + kk;
        // the entries this lane will update, requested before the products (clamped addresses, masked at the store)
        double* dst[4];
        double old[4];
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int io = 16 * bi + kk + 4 * r, jo = 16 * bj + i16;
            ok[r] = io < tr && jo < tc && jo <= io;
            dst[r] = Wm + (size_t)(k1 + (ok[r] ? io : 0)) * DA + k1 + (ok[r] ? jo : 0);
            old[r] = *dst[r];
        }
        f64x4 acc = zero4d();
#pragma unroll
        for (int sidx = 0; sidx < NB / 4; ++sidx) acc = mfma16d(pa[4 * sidx], pb[4 * sidx], acc);
        // D: col = lane & 15, row = (lane >> 4) + 4 r
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (ok[r]) *dst[r] = old[r] - acc[r];
    }
}
// only_bad != nullptr: the launch behind the one-launch-per-phase factorisation below -- tasks whose flag is 0 are done; the others
// (a NaN in the solution: the ridge term was too small) start over at the second attempt, reg x 10, exactly as they would have here.
template <int NB>
__global__ void __launch_bounds__(FITW_NT) k_fit_wide(SampleArgs a, int NBLK, double* scratch, const int* only_bad) {
    constexpr int PS = NB + 1;
    PROMP_SMEM_DECL;
#ifdef PROMP_DEV_STAMPS
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tph = promp_clock();
#define FITW_PHASE(i) do { const unsigned long long now_ = promp_clock(); ph[i] += now_ - tph; tph = now_; } while (0)
#else
#define FITW_PHASE(i) do { } while (0)
#endif
    const int D = a.D, DA = D + 1, NT = FITW_NT;
    const int tid = threadIdx.x, task = blockIdx.x, lane = tid & 63, w = wave_uniform(tid >> 6);
    double* Pn = (double*)PROMP_SMEM_PTR;     // panel [DA - k0 (+ 16)][33]
    double* yv = Pn + (size_t)(DA + 16) * PS;
    double* wv = yv + DA;
    double* dg = wv + DA;
    double* rdp = dg + DA;                    // 1 / L[c][c] of the current panel's diagonal block
    int* flag = (int*)(rdp + NB);
    double* G = scratch + (size_t)task * 2 * DA * DA;
    double* Wm = G + (size_t)DA * DA;
    // (G, and G + reg I as the work matrix of the first attempt, were written by k_gram_sum_wide)
    const float rDA = 1.0f / (float)DA;
    if (only_bad != nullptr && !only_bad[task]) return;          // (uniform over the workgroup)
    const int first_attempt = only_bad != nullptr ? 1 : 0;
    double reg = first_attempt ? a.reg * 10.0 : a.reg;
    for (int attempt = first_attempt; attempt < 5; ++attempt) {
        if (attempt > 0) {            // a retry starts over from G with the larger ridge term
            for (int e = tid; e < DA * DA; e += NT) {
                const int i = (int)(((float)e + 0.5f) * rDA), j = e - i * DA;
                Wm[e] = G[e] + ((i == j && i < D) ? reg : 0.0);
            }
        }
        __syncthreads();
        FITW_PHASE(1);
        for (int k0 = 0; k0 < D; k0 += NB) {
            const int nb = (D - k0) < NB ? (D - k0) : NB;   // columns of this panel
            const int nr = DA - k0;                                  // rows k0..D (the last one is the right-hand side)
            chol_panel_load<NB, 16>(Pn, Wm, DA, k0, k0, nr, nb, tid);       // (16 rows of zeros behind the panel)
            __syncthreads();
            FITW_PHASE(2);
            if (w == 0) chol_diag_block<NB, true>(Pn, rdp, dg + k0, nb, lane);
            __syncthreads();
            FITW_PHASE(3);
            chol_rows_below<NB>(Pn, rdp, nb, nr - nb, tid);
            __syncthreads();
            FITW_PHASE(4);
            chol_panel_store<NB>(Wm, Pn, DA, k0, nr, nb, false, tid);       // (the diagonal stays in dg[])
            // all waves of the workgroup: wave w takes tiles w, w + 8, ...
            if (k0 + nb < D) chol_trailing_update<NB>(Wm, Pn, nb, D, k0 + nb, w, FITW_NT / 64, lane);
            __syncthreads();
            FITW_PHASE(5);
        }
        // ---- back substitution L^T w = z, z = row D of the factor, 32 rows of L at a time (the reciprocals of the factor's diagonal
        //      take the diagonal's place: one division per thread here instead of one per block on wave 0's chain)
        for (int e = tid; e < D; e += NT) {
            yv[e] = Wm[(size_t)D * DA + e];
            dg[e] = 1.0 / dg[e];
        }
        fitw_back_substitute<NB>(Wm, D, DA, yv, wv, dg, Pn, tid, lane, w);     // (the panel's LDS is free: two triangles)
        FITW_PHASE(6);
        if (tid == 0) *flag = 0;
        __syncthreads();
        const int bad = fit_any_nan<false>(wv, D, flag, tid, NT);
        __syncthreads();
        if (!bad) break;
        reg *= 10.0;
    }
    for (int e = tid; e < D; e += NT) a.coeffs[(long long)task * a.coeff_stride + e] = wv[e];
#ifdef PROMP_DEV_STAMPS
    if (task == 0 && tid == 0)
        printf("k_fit_wide cycles: entry %llu | retry init %llu | panel load %llu | diagonal block %llu | rows below %llu | store + update %llu | back substitution %llu\n",
               ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6]);
#endif
}

// ---------------------------------------------------------------------------------------------
// The same factorisation with ONE LAUNCH PER PHASE, for matrices so large that one compute unit per task is the wrong shape
// (Humanoid: D = 756, 48 panels of 16 columns; the rank-16 update of a 740 x 740 trailing matrix is 1100 tiles of 16 x 16 per
// panel -- in k_fit_wide 8 waves of ONE CU walk them while 216 CUs idle: 3.5 ms per fit at 40 tasks):
//   k_fitw_panel  (grid = tasks)                    panel k0: diagonal block, rows below, factored panel back into the work matrix
//   k_fitw_update (grid = tasks x FITW_UPD_SPLIT)   trailing matrix -= panel panel^T on the FP64 matrix cores, all CUs
//   ... per panel, then
//   k_fitw_back   (grid = tasks)                    back substitution, NaN check -> coefficients, or bad[task] = 1
//   k_fit_wide(only_bad)                            the (rare) retries with a larger ridge term, unchanged
// Same elimination order and the same arithmetic per entry as k_fit_wide (every trailing entry takes one 16-term MFMA sum per
// panel whichever wave computes it): bit-identical coefficients.  The diagonal of the factor is kept on the work matrix' diagonal.
// ---------------------------------------------------------------------------------------------
PROMP_HD size_t fitw_panel_smem(int D, int nb) { return sizeof(double) * ((size_t)(D + 1 + 16) * (nb + 1) + nb + 2); }
PROMP_HD size_t fitw_back_smem(int D, int nb) { return sizeof(double) * ((size_t)3 * (D + 1) + 2 * nb * (nb + 1) + 2); }

template <int NB>
__global__ void __launch_bounds__(FITW_NT) k_fitw_panel(SampleArgs a, double* scratch, int k0) {
    constexpr int PS = NB + 1;
    PROMP_SMEM_DECL;
    const int D = a.D, DA = D + 1;
    const int tid = threadIdx.x, task = blockIdx.x, lane = tid & 63, w = wave_uniform(tid >> 6);
    double* Pn = (double*)PROMP_SMEM_PTR;             // [DA - k0][PS]
    double* rdp = Pn + (size_t)(DA + 16) * PS;        // 1 / L[c][c] of the diagonal block
    double* Wm = scratch + (size_t)task * 2 * DA * DA + (size_t)DA * DA;
    const int nb = (D - k0) < NB ? (D - k0) : NB;     // columns of this panel
    const int nr = DA - k0;                           // rows k0..D (the last one is the right-hand side)
    chol_panel_load<NB, 0>(Pn, Wm, DA, k0, k0, nr, nb, tid);
    __syncthreads();
    if (w == 0) chol_diag_block<NB, false>(Pn, rdp, nullptr, nb, lane);
    __syncthreads();
    chol_rows_below<NB>(Pn, rdp, nb, nr - nb, tid);
    __syncthreads();
    chol_panel_store<NB>(Wm, Pn, DA, k0, nr, nb, true, tid);                // (the diagonal with it: k_fitw_back reads it there)
}

template <int NB>
__global__ void __launch_bounds__(FITW_NT) k_fitw_update(SampleArgs a, double* scratch, int k0) {
    PROMP_SMEM_DECL;
    const int D = a.D, DA = D + 1;
    const int tid = threadIdx.x, task = blockIdx.x, lane = tid & 63, w = wave_uniform(tid >> 6);
    double* Pn = (double*)PROMP_SMEM_PTR;             // [tr + 16][PS]: the factored panel's rows below its diagonal block
    double* Wm = scratch + (size_t)task * 2 * DA * DA + (size_t)DA * DA;
    const int nb = (D - k0) < NB ? (D - k0) : NB;
    const int k1 = k0 + nb;
    chol_panel_load<NB, 16>(Pn, Wm, DA, k1, k0, DA - k1, nb, tid);
    __syncthreads();
    // the tiles dealt to all waves of the task's workgroups
    chol_trailing_update<NB>(Wm, Pn, 0, D, k1, w + (FITW_NT / 64) * (int)blockIdx.y, (FITW_NT / 64) * (int)gridDim.y, lane);
}

template <int NB>
__global__ void __launch_bounds__(FITW_NT) k_fitw_back(SampleArgs a, double* scratch, int* bad) {
    PROMP_SMEM_DECL;
    const int D = a.D, DA = D + 1, NT = FITW_NT;
    const int tid = threadIdx.x, task = blockIdx.x, lane = tid & 63, w = wave_uniform(tid >> 6);
    double* yv = (double*)PROMP_SMEM_PTR;
    double* wv = yv + DA;
    double* rdv = wv + DA;                    // 1 / diag(L)
    double* tri = rdv + DA;                   // two triangles of the factor's diagonal blocks
    int* flag = (int*)(tri + 2 * NB * (NB + 1));
    const double* Wm = scratch + (size_t)task * 2 * DA * DA + (size_t)DA * DA;
    // ---- back substitution L^T w = z, z = row D of the factor, NB rows of L at a time
    for (int e = tid; e < D; e += NT) {
        yv[e] = Wm[(size_t)D * DA + e];
        rdv[e] = 1.0 / Wm[(size_t)e * DA + e];
    }
    if (tid == 0) *flag = 0;
    fitw_back_substitute<NB>(Wm, D, DA, yv, wv, rdv, tri, tid, lane, w);       // (its barriers cover the flag)
    const int isbad = fit_any_nan<false>(wv, D, flag, tid, NT);
    if (tid == 0) bad[task] = isbad;
    if (!isbad)
        for (int e = tid; e < D; e += NT) a.coeffs[(long long)task * a.coeff_stride + e] = wv[e];
}
