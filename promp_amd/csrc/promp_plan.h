// promp_plan.h -- host planning: every decision about WHAT the GPU runs, and nothing that runs there.
//
//   shapes       which network shapes a context accepts, how narrow hidden layers are embedded in the instantiated widths, which
//                family of pass kernels serves a (padded) shape
//   Stage A      which Gram and fit kernels promp_process_samples launches for a baseline kind and an observation width
//   step tables  the work tables, the chain kernels' segment table, the time indices and the task row offsets of a sampling step
//   selections   which paths of a step a subsampled constraint product keeps, and the layout of the compact slab that holds them
//   partitions   a step's paths dealt to the compact slabs of its minibatches
//   table blocks the one block of ints that holds a copy launch's table and the pass tables of the compact slabs it fills
//   outer step   the update rule, its arguments and the gradient clip of the final stage, and which kernel family runs it
//   switches     the PROMP_* environment switches the above depend on, read once
//
// HIP-free: the C ABI header and the standard library only, so plain `g++ -std=c++17` compiles it alone and
// tests/host/plan_check.cpp runs every function below under AddressSanitizer / UBSan in milliseconds (tests/test_plan_host.py).
// The kernel headers include it for the constants and sizing helpers they share with the plan; promp_hip.hip for everything.
#pragma once
#include "../../include/promp_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// helpers the kernels call as well: host + device under hipcc, plain inline for a host compiler (the emulator build among them)
#ifdef __HIPCC__
#define PROMP_PLAN_HD __host__ __device__ inline
#else
#define PROMP_PLAN_HD inline
#endif

// A refused plan: the return code, and the message for promp_last_error() through `why`
inline int plan_fail(std::string* why, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (why) *why = buf;
    return code;
}

// ---- switches ------------------------------------------------------------------------------------------------------------
// The A/B switches of the measurements and the tests' compute-unit cap, read from the environment once per context
// (promp_ctx_create).  PROMP_SIDE_PRIO is a property of a stream and is read where that stream is made.
struct PlanSwitches {
    bool fit_one_launch = false;   // PROMP_FIT_ONE_LAUNCH=1: k_fit_wide alone at every width (A/B runs against the per-phase launches)
    bool gram_untiled = false;     // PROMP_GRAM_UNTILED=1: k_gram_wide at every width (A/B runs against k_gram_tiled)
    bool gramt_single = false;     // PROMP_GRAMT_SINGLE=1: k_gram_tiled with one feature tile (A/B runs against the double-buffered rounds)
    bool wide_fp32 = false;        // PROMP_WIDE_FP32 != 0: (128,128) stays on the exact-FP32 cooperative kernels
    bool gen_fp32 = false;         // PROMP_GEN_FP32=1: the layer-by-layer GEMMs on the exact-FP32 kernels
    int max_cus = 0;               // PROMP_MAX_CUS > 0: work tables for at most this many compute units (tests: a wave then walks
                                   // several tiles of a small batch)
    bool outer_generic = false;    // PROMP_OUTER_GENERIC=1: the general final-stage kernels under default settings too (A/B runs and
                                   // the bit-for-bit test against the plain ones)
};
inline PlanSwitches plan_switches_from_env() {
    auto is1 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
    PlanSwitches sw;
    sw.fit_one_launch = is1("PROMP_FIT_ONE_LAUNCH");
    sw.gram_untiled = is1("PROMP_GRAM_UNTILED");
    sw.gramt_single = is1("PROMP_GRAMT_SINGLE");
    sw.gen_fp32 = is1("PROMP_GEN_FP32");
    sw.outer_generic = is1("PROMP_OUTER_GENERIC");
    { const char* e = getenv("PROMP_WIDE_FP32"); sw.wide_fp32 = e && atoi(e) != 0; }
    { const char* e = getenv("PROMP_MAX_CUS"); sw.max_cus = e ? atoi(e) : 0; }
    return sw;
}

// ---- shapes --------------------------------------------------------------------------------------------------------------
#define GEN_MAX_LIN 5          // linear layers: up to 4 hidden + the output layer
#define GEN_MAX_N 256          // widest layer output (4 waves x 4 column blocks of 16)
#define GEN_MAX_A 64
#define PROMP_ETA_MAX 8        // most inner gradient steps a context is created for
#define PROMP_LINFEAT_MAX_O 480     // LinearFeatureBaseline on the device: 2 obs_dim + 5 <= 965 columns (16 feature rows + their observations in LDS)

// waves per workgroup of k_pass / k_chain_hvp (one per SIMD: 512 registers per lane)
constexpr int CHAIN_NW_HVP = 4;
// layer-1 k-steps k_chain_hvp is instantiated for (4 observation entries per step, zero-padded)
inline int chain_ksteps(int obs_dim) { return obs_dim <= 8 ? 2 : obs_dim <= 20 ? 5 : 8; }
// observation blocks of 16 the k_wide_* kernels are instantiated for
inline int wide_nob(int obs_dim) { return obs_dim <= 32 ? 2 : obs_dim <= 64 ? 4 : 8; }
inline int wb_nko(int cls) { return cls == 1 ? 4 : cls == 2 ? 7 : 8; }      // K = 16 steps of the observation per class

// hidden_sizes of a context: promp_dims carries up to four widths (n_hidden == 0: the two-layer struct of ABI 2)
struct HiddenList {
    int n;
    int h[4];
};
inline HiddenList hidden_list(const promp_dims* d) {
    HiddenList L;
    L.n = d->n_hidden > 0 ? d->n_hidden : 2;
    L.h[0] = d->hidden1; L.h[1] = d->hidden2; L.h[2] = d->hidden3; L.h[3] = d->hidden4;
    return L;
}
inline bool policy_shape_generic(const promp_dims* d) {   // layer-by-layer kernels (promp_kernels_generic.h): everything the fused ones do not cover
    const HiddenList L = hidden_list(d);
    return L.n != 2 || d->obs_dim > 128 || d->act_dim > 8 || d->hidden1 > 128 || d->hidden2 > 128 || d->hidden_act != PROMP_ACT_TANH;      // (an output nonlinearity sits in the upper bits: != too)
}

inline int check_dims(const promp_dims* d, std::string* why) {
    if (!d) return plan_fail(why, -1, "dims is NULL");
    if (d->n_tasks < 1 || d->n_tasks_global < d->n_tasks) return plan_fail(why, -1, "bad task counts (%d local, %d global)", d->n_tasks, d->n_tasks_global);
    if (d->obs_dim < 1 || d->obs_dim > 1024) return plan_fail(why, -1, "obs_dim %d unsupported (1..1024)", d->obs_dim);
    if (d->act_dim < 1 || d->act_dim > GEN_MAX_A) return plan_fail(why, -1, "act_dim %d unsupported (1..%d)", d->act_dim, GEN_MAX_A);
    const HiddenList L = hidden_list(d);
    if (d->n_hidden < 0 || L.n > 4) return plan_fail(why, -1, "hidden_sizes of length %d unsupported (1..4 hidden layers)", L.n);
    for (int l = 0; l < L.n; ++l)
        if (L.h[l] < 1 || L.h[l] > GEN_MAX_N)
            return plan_fail(why, -1, "hidden size %d (layer %d) unsupported: tanh layers of 1..%d units.  Two layers of up to 128 units run on the fused "
                             "kernels (narrower ones zero-padded on the instantiated widths: every combination of {32, 64} for obs_dim <= 32, "
                             "(64,64) / (128,128) otherwise); wider layers and other depths on the layer-by-layer kernels", L.h[l], l, GEN_MAX_N);
    if ((d->hidden_act & 0xff) > PROMP_ACT_IDENTITY || d->hidden_act < 0)
        return plan_fail(why, -1, "hidden_act %d unknown (0 tanh, 1 relu, 2 identity)", d->hidden_act & 0xff);
    if ((d->hidden_act >> PROMP_OUT_ACT_SHIFT) > PROMP_OUT_ACT_RELU)
        return plan_fail(why, -1, "output nonlinearity %d unknown (0 none, 1 tanh, 2 relu)", d->hidden_act >> PROMP_OUT_ACT_SHIFT);
    if (d->num_inner_steps < 1 || d->num_inner_steps > PROMP_ETA_MAX) return plan_fail(why, -1, "num_inner_steps must be in [1, %d]", PROMP_ETA_MAX);
    if (d->max_rows < 1 || d->max_paths < 1) return plan_fail(why, -1, "max_rows / max_paths must be positive");
    return 0;
}

// The flattened parameter vector of a two-hidden-layer policy, in the order policies/base.py:271-277 fixes: hidden_0 kernel [O][H1]
// at 0, then hidden_0 bias, hidden_1 kernel [H1][H2], hidden_1 bias, output kernel [H2][A], output bias, log_std; NP entries.
// Every kernel that indexes a parameter vector, a direction or a partial row of such a policy takes its offsets from here, and so
// do param_count, remap_params and the hidden_0 block of k_vec_absmax (tests/host/plan_check.cpp ties them to each other).
struct Mlp2Layout {
    int b1, W2, b2, W3, b3, ls, NP;
};
// (always inlined: the kernels' force-inlined helpers call it, and they are inlined before the optimiser looks at an ordinary call)
PROMP_PLAN_HD __attribute__((always_inline)) Mlp2Layout mlp2_layout(int O, int H1, int H2, int A) {
    Mlp2Layout l;
    l.b1 = O * H1;
    l.W2 = l.b1 + H1;
    l.b2 = l.W2 + H1 * H2;
    l.W3 = l.b2 + H2;
    l.b3 = l.W3 + H2 * A;
    l.ls = l.b3 + A;
    l.NP = l.ls + A;
    return l;
}

inline int param_count(const promp_dims* d) {
    const HiddenList L = hidden_list(d);
    if (L.n == 2) return mlp2_layout(d->obs_dim, L.h[0], L.h[1], d->act_dim).NP;
    int n = 0, in = d->obs_dim;
    for (int l = 0; l < L.n; ++l) {
        n += in * L.h[l] + L.h[l];
        in = L.h[l];
    }
    return n + in * d->act_dim + d->act_dim + d->act_dim;
}

inline int feature_dim(const promp_dims* d, int kind) {
    if (kind == PROMP_BASELINE_LINEAR_FEATURE) return 2 * d->obs_dim + 4;
    if (kind == PROMP_BASELINE_LINEAR_TIME) return 4;
    return 0;
}

// The kernels are instantiated for hidden widths from {32, 64} in any combination (obs_dim <= 32) and for (64,64) / (128,128).
// Any other pair of widths up to 128 runs EMBEDDED in the next instantiated shape: the extra hidden units have zero incoming and
// outgoing weights and zero bias, so they output tanh(0) = 0, receive a zero cotangent, and every gradient / Hessian-vector entry
// that belongs to them is exactly zero -- they stay zero under the inner steps and under Adam.  Parameter vectors cross the C ABI in
// the caller's (unpadded) layout (policies/networks/mlp.py:5-62 takes any hidden_sizes; policies/base.py:271-277 fixes the order).
inline void pad_dims(const promp_dims* u, promp_dims* p) {
    *p = *u;
    if (policy_shape_generic(u)) return;          // the layer-by-layer kernels take any width as it is
    auto up = [](int h) { return h <= 32 ? 32 : h <= 64 ? 64 : 128; };
    int a = up(u->hidden1), b = up(u->hidden2);
    if (u->obs_dim > 32) a = b = std::max(std::max(a, b), 64);
    else if (a == 128 || b == 128) a = b = 128;
    p->hidden1 = a;
    p->hidden2 = b;
}
// one parameter vector between the caller's layout (du) and the padded one (dp); to_padded: dst must arrive zeroed
inline void remap_params(const promp_dims& du, const promp_dims& dp, const float* src, float* dst, bool to_padded) {
    const int O = du.obs_dim, A = du.act_dim, h1 = du.hidden1, h2 = du.hidden2, H1 = dp.hidden1, H2 = dp.hidden2;
    const Mlp2Layout lu = mlp2_layout(O, h1, h2, A), lp = mlp2_layout(O, H1, H2, A);
    // one block: nrows_u x cols_u entries of the caller's vector at ou, embedded in rows of cols_p entries at op
    auto rows = [&](int ou, int op, int nrows_u, int cols_u, int cols_p) {
        for (int r = 0; r < nrows_u; ++r)
            for (int cc = 0; cc < cols_u; ++cc) {
                if (to_padded) dst[op + (size_t)r * cols_p + cc] = src[ou + (size_t)r * cols_u + cc];
                else dst[ou + (size_t)r * cols_u + cc] = src[op + (size_t)r * cols_p + cc];
            }
    };
    rows(0, 0, O, h1, H1);             // hidden_0/kernel
    rows(lu.b1, lp.b1, 1, h1, H1);     // hidden_0/bias
    rows(lu.W2, lp.W2, h1, h2, H2);    // hidden_1/kernel
    rows(lu.b2, lp.b2, 1, h2, H2);     // hidden_1/bias
    rows(lu.W3, lp.W3, h2, A, A);      // output/kernel
    rows(lu.b3, lp.b3, 1, A, A);       // output/bias
    rows(lu.ls, lp.ls, 1, A, A);       // log_std
}

// which kernels run the policy passes of a context (promp_ctx_create chooses once, from the padded dims)
enum class PassFamily {
    Chain,       // register-chained k_pass / k_chain_hvp (promp_kernels_chain.h, promp_kernels_pass.h): widths from {32, 64}, obs_dim <= 32
    CoopFp32,    // cooperative exact-FP32 k_wide_* (promp_kernels_policy_wide.h): (64,64) with obs_dim > 32, (128,128) outside CoopSplit
    CoopSplit,   // cooperative k_wb_* on the BF16 matrix pipe (promp_kernels_wide_bf16.h): (128,128) with obs_dim <= 127
    Layered,     // layer-by-layer k_gen_* / k_gb_* (promp_kernels_generic*.h): every shape policy_shape_generic() names
};
struct FamilyPlan {
    PassFamily family;
    int wb_cls;                  // CoopSplit: the observation class 1..3 = (NKO, NXB) = (4,2) (7,4) (8,4): obs_dim <= 63 / 111 / 127
};
// The pass family of PADDED dims.  Every shape check_dims accepts falls into exactly one, so launch_pass has a kernel for every
// context:
//   - policy_shape_generic() (not two layers, obs_dim > 128, act_dim > 8, a width > 128, not tanh): Layered, dims as given;
//   - otherwise pad_dims has made the widths (32|64, 32|64) with obs_dim <= 32: Chain; or equal widths of 64 / 128 when
//     obs_dim > 32 or a width exceeded 64: the cooperative kernels, CoopSplit for (128,128) with obs_dim <= 127 unless
//     PROMP_WIDE_FP32=1 keeps the exact-FP32 CoopFp32 (the A/B switch of the measurements), CoopFp32 for the rest:
//     (128,128) with obs_dim 128 and (64,64) with obs_dim > 32.
inline FamilyPlan pass_family(const promp_dims* d, const PlanSwitches& sw) {
    if (policy_shape_generic(d)) return {PassFamily::Layered, 0};
    if (d->obs_dim <= 32 && d->hidden1 != 128) return {PassFamily::Chain, 0};
    if (d->hidden1 == 128 && d->obs_dim <= 127 && !sw.wide_fp32)
        return {PassFamily::CoopSplit, d->obs_dim <= 63 ? 1 : d->obs_dim <= 111 ? 2 : 3};
    return {PassFamily::CoopFp32, 0};
}

// ---- Stage A: the Gram and fit kernels of promp_process_samples ---------------------------------------------------------------
// k_gram<NBLK> instances (feature blocks of 16) and k_fit_wave<DT> instances (ascending: the first with D + 1 <= DT runs)
#define PROMP_GRAM_ALL(X) X(1) X(2) X(3) X(4) X(5)
#define PROMP_FITWV_ALL(X) X(12) X(45) X(48) X(64)

#define FITWV_CS 65        // doubles between the factor's columns in LDS (k_fit_wave: 64 lanes + 1: a lane walking down its own
                           // column -- the back substitution's operands -- is then on its own pair of banks)
PROMP_PLAN_HD size_t fitwv_aux(int dt) { return (size_t)dt * FITWV_CS + 2 + 64; }     // the factor by columns + 1 / L[j][j]

#define GRAMW_PPW 20     // pairs per wave: 8 * 20 >= 17 * 18 / 2 (NBLK <= 17, D <= 271) in one workgroup; more blocks: the pair list is
                         // cut into gridDim.y slices of at most 160 (gramw_slices), one workgroup per work item and slice
PROMP_PLAN_HD int gramw_fs(int NBLK) { return (NBLK % 2 == 1) ? 16 * NBLK : 16 * NBLK + 16; }
PROMP_PLAN_HD size_t gramw_smem(int NBLK, int O, int rows) {
    (void)O;
    return sizeof(double) * (size_t)(rows * gramw_fs(NBLK));      // the feature tile
}
// rows per round: 64 where the feature tile + raw observations fit the 160 KB of LDS (Ant: 151 KB), else 32, else 16
PROMP_PLAN_HD int gramw_rows(int NBLK, int O) {
    return gramw_smem(NBLK, O, 64) <= 160 * 1024 ? 64 : gramw_smem(NBLK, O, 32) <= 160 * 1024 ? 32 : 16;
}
PROMP_PLAN_HD int gramw_slices(int NBLK) { return (NBLK * (NBLK + 1) / 2 + 8 * GRAMW_PPW - 1) / (8 * GRAMW_PPW); }

#define GRAMT_MIN_NBLK 13
#define GRAMT_TB 3
#define GRAMT_NWV 16
#define GRAMT_NLD 8
struct GramtMap {        // one-slice launches: wave -> square (255: none) and which part of a diagonal square (GRAMT_*)
    unsigned char rect[16], part[16];
};
enum { GRAMT_FULL = 0, GRAMT_DIAG = 1, GRAMT_DIAG_TOP = 2, GRAMT_DIAG_REST = 3 };
PROMP_PLAN_HD int gramt_nb(int NBLK) { return (NBLK + GRAMT_TB - 1) / GRAMT_TB; }
PROMP_PLAN_HD int gramt_fs(int NBLK) {       // 16 x odd: the four k-rows of a step land on disjoint banks
    const int nc = GRAMT_TB * gramt_nb(NBLK);
    return (nc % 2 == 1) ? 16 * nc : 16 * nc + 16;
}
PROMP_PLAN_HD int gramt_nrect(int NBLK) { return gramt_nb(NBLK) * (gramt_nb(NBLK) + 1) / 2; }
// rows per round and single / double tile: two tiles of 32 or 16 rows where they fit LDS (and a round's observations the
// threads' request registers: cap = NT * NLD elements) -- the build of round r + 1 then runs beside the products of round r
// behind ONE barrier per round; `single` (PROMP_GRAMT_SINGLE=1, the A/B switch) or nothing fitting twice: one tile of 32 / 16 rows,
// the build between two barriers.
PROMP_PLAN_HD void gramt_cfg(int NBLK, int O, int cap, bool single, int* rows, int* db) {
    const size_t row_bytes = sizeof(double) * (size_t)gramt_fs(NBLK), lds = 160 * 1024;
    if (!single)
        for (int r = 32; r >= 16; r >>= 1)      // (two tiles of 8 rows measured slower than one of 16 at Humanoid's width: 2.37 vs 2.21 ms)
            if (2 * r * row_bytes <= lds && r * O <= cap) { *rows = r; *db = 1; return; }
    *rows = (32 * row_bytes <= lds && 32 * O <= cap) ? 32 : 16;
    *db = 0;
}

#define FITW_NB 32         // panel width where the panel fits LDS (D <= ~580); wider matrices take 16-column panels
#define FITW_NT 512        // 8 waves: two per SIMD, 256 registers each (a row of the diagonal block / of the solve lives in 64 of them)
PROMP_PLAN_HD size_t fitw_smem(int D, int nb) {
    const size_t DA = D + 1, panel = (DA + 16) * (size_t)(nb + 1);       // (16 spare rows: the last 16-row tile of the update reads zeros)
    return sizeof(double) * (panel + 3 * DA + nb + 2);
}
PROMP_PLAN_HD int fitw_nb(int D) { return fitw_smem(D, FITW_NB) <= 160 * 1024 ? FITW_NB : 16; }
// workgroups per task of k_gram_sum_wide (the split grows with the matrix: see there)
PROMP_PLAN_HD int fitw_sum_split(int NBLK) { return NBLK >= 32 ? 32 : NBLK >= 13 ? 16 : 8; }
#define FITW_UPD_SPLIT 6          // 40 tasks x 6 = 240 workgroups
#define FITW_ML_MIN_D 400         // below: k_fit_wide (8 panels at Ant's 226 columns are a chain of dependent steps, not tile work)

enum class GramKernel { None, Small, Wide, Tiled };    // none (ZeroBaseline) | k_gram<gram_nblk> | k_gram_wide | k_gram_tiled
enum class FitKernel { None, Wave, Block, Wide };      // none | k_fit_wave<fit_arg> | k_fit | k_fit_wide<fit_arg>
struct SamplePlan {
    int nblk = 0;                          // blocks of 16 among the D + 1 columns (the features and the target)
    GramKernel gram = GramKernel::None;
    int gram_nblk = 0;                     // Small: the template argument
    int gram_slices = 1;                   // Wide: pair slices, Tiled: slices of GRAMT_NWV squares (gridDim.y)
    int gram_rows = 0, gram_db = 0;        // Wide / Tiled: rows per round; Tiled: two feature tiles
    FitKernel fit = FitKernel::None;
    int fit_arg = 0;                       // Wave: DT, Wide: the panel width NB
    bool fit_phases = false;               // Wide: k_fitw_panel / k_fitw_update / k_fitw_back<NB> in front of k_fit_wide<NB>
    int sum_split = 0;                     // Wide: workgroups per task of k_gram_sum_wide
};
// The kernels of one promp_process_samples: baseline kind, observation width O, D = feature_dim of the kind.
inline int sample_plan(int kind, int O, int D, const PlanSwitches& sw, SamplePlan* p, std::string* why) {
    *p = SamplePlan();
    if (kind == PROMP_BASELINE_LINEAR_FEATURE && O > PROMP_LINFEAT_MAX_O)
        return plan_fail(why, -1, "LinearFeatureBaseline's fit is sized for obs_dim <= %d (%d here: %d feature columns); fit LinearTimeBaseline / no "
                         "baseline on the device, or hand advantages in through promp_set_advantages", PROMP_LINFEAT_MAX_O, O, 2 * O + 5);
    if (kind == PROMP_BASELINE_ZERO) return 0;
    const int nblk = (D + 1 + 15) / 16, DA = D + 1;
    p->nblk = nblk;
    // k_gram<NBLK> stages raw observation rows of at most 32 floats (LinearTimeBaseline reads no observations: any obs_dim)
    if (nblk <= 5 && (O <= 32 || kind != PROMP_BASELINE_LINEAR_FEATURE)) {
        p->gram = GramKernel::Small;
        p->gram_nblk = nblk;
        // one wave per task while a row of the work matrix fits a wave's lanes (D + 1 <= 64); else one workgroup per task
        // (45: obs_dim 20)
        p->fit = FitKernel::Block;
#define PROMP_PLAN_FITWV(DT) if (p->fit == FitKernel::Block && DA <= DT) { p->fit = FitKernel::Wave; p->fit_arg = DT; }
        PROMP_FITWV_ALL(PROMP_PLAN_FITWV)
#undef PROMP_PLAN_FITWV
        return 0;
    }
    // 13 blocks and more (obs_dim >= 94; Ant: 15, Humanoid: 48): a square of 3 x 3 blocks per wave, operands reused in
    // registers (k_gram_tiled); fewer blocks make too few squares to fill a compute unit: k_gram_wide
    if (nblk >= GRAMT_MIN_NBLK && !sw.gram_untiled) {
        p->gram = GramKernel::Tiled;
        p->gram_slices = (gramt_nrect(nblk) + GRAMT_NWV - 1) / GRAMT_NWV;
        gramt_cfg(nblk, O, 64 * GRAMT_NWV * GRAMT_NLD, sw.gramt_single, &p->gram_rows, &p->gram_db);
    } else {
        // (more than 17 blocks -- obs_dim > 133: the pair list is cut into slices of <= 160, one workgroup per work item and slice)
        p->gram = GramKernel::Wide;
        p->gram_slices = gramw_slices(nblk);
        p->gram_rows = gramw_rows(nblk, O);
    }
    p->fit = FitKernel::Wide;
    p->fit_arg = fitw_nb(D);
    p->fit_phases = D >= FITW_ML_MIN_D && !sw.fit_one_launch;      // one launch per phase: all CUs in the trailing updates
    p->sum_split = fitw_sum_split(nblk);
    return 0;
}

// k_gram_tiled, one slice (at most GRAMT_NWV squares): share the squares out over the waves so that the four SIMDs of a compute
// unit carry about the same number of matrix instructions per k-step (wave w of a workgroup runs on SIMD w mod 4).  Waves to
// spare take halves of diagonal squares (first row of the triangle / the rest: 3 + 3 products at TB = 3) -- Ant's 15 squares on
// 16 waves: 10 x 9 + 4 x 6 + 2 x 3 products = 30 per SIMD.  Longest first, each to the least loaded SIMD that still has a wave
// free.  More squares than waves: slices in list order, diagonal squares whole (the kernel ignores the map).
inline void gramt_balance(int nblk, int nwv, GramtMap* map) {
    const int nb = gramt_nb(nblk), nr = gramt_nrect(nblk), TB = GRAMT_TB;
    memset(map->rect, 255, sizeof map->rect);
    memset(map->part, GRAMT_DIAG, sizeof map->part);
    if (nr > nwv || nwv > 16) return;
    struct Piece { int rect, part, cost; };
    std::vector<Piece> pieces;
    int spare = nwv - nr;
    for (int bi = 0, r = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj, ++r) {
            if (bi != bj) pieces.push_back({r, GRAMT_FULL, TB * TB});
            else if (spare > 0) {
                pieces.push_back({r, GRAMT_DIAG_TOP, TB});
                pieces.push_back({r, GRAMT_DIAG_REST, TB * (TB + 1) / 2 - TB});
                --spare;
            } else pieces.push_back({r, GRAMT_DIAG, TB * (TB + 1) / 2});
        }
    std::stable_sort(pieces.begin(), pieces.end(), [](const Piece& x, const Piece& y) { return x.cost > y.cost; });
    int slots[4] = {0, 0, 0, 0}, load[4] = {0, 0, 0, 0}, next[4] = {0, 1, 2, 3};
    for (int w = 0; w < nwv; ++w) slots[w & 3]++;
    for (const Piece& pc : pieces) {
        int q = -1;
        for (int t = 0; t < 4; ++t)
            if (slots[t] > 0 && (q < 0 || load[t] < load[q])) q = t;
        map->rect[next[q]] = (unsigned char)pc.rect;
        map->part[next[q]] = (unsigned char)pc.part;
        next[q] += 4; slots[q]--; load[q] += pc.cost;
    }
}

// ---- step tables ---------------------------------------------------------------------------------------------------------
struct WorkItem {
    int task, row_begin, row_end, pad;
};
struct ChainSeg {
    int task, tile0, ntiles, pad;   // 16-row tiles [tile0, tile0 + ntiles) of the task; slot = index of the segment
};
// Everything the device reads about the layout of one sampling step, as the host builds it (set_step_layout copies each array
// to its device buffer)
struct StepTables {
    std::vector<int> pro, tpo;             // the caller's path_row_offsets [paths + 1] / task_path_offsets [tasks + 1]
    std::vector<int> path_task, row_t;     // [paths] the task of a path; [rows] the time index of a row inside its path
    std::vector<int> tro;                  // [tasks + 1] task row offsets
    std::vector<WorkItem> work[2];         // [0]: one workgroup per CU (wide passes, gram, fit), [1]: two per CU (k_normalize)
    std::vector<int> two[2];               // [tasks + 1] each: the work items of a task
    std::vector<ChainSeg> segs;            // segment table of k_pass / k_chain_hvp
    std::vector<int> wg_off;               // [workgroups + 1]: the segments of a workgroup
    std::vector<int> slot_chain;           // [tasks + 1]: partial rows (= segments) of each task
};
// Offsets, time indices, the two work tables and the segment table of one sampling step from the caller's offsets: tpo [M + 1],
// pro [n_paths + 1].  Refuses malformed offsets before anything is indexed by them.
inline int build_step_tables(int n_cus, int max_work, int max_rows, int max_paths, int M, int n_paths, const int32_t* tpo,
                             const int32_t* pro, StepTables* out, std::string* why) {
    if (n_paths < 1 || n_paths > max_paths) return plan_fail(why, -1, "n_paths %d outside [1, max_paths=%d]", n_paths, max_paths);
    if (tpo[0] != 0 || tpo[M] != n_paths) return plan_fail(why, -1, "task_path_offsets must start at 0 and end at n_paths");
    if (pro[0] != 0) return plan_fail(why, -1, "path_row_offsets must start at 0");
    const int R = pro[n_paths];
    if (R < 1 || R > max_rows) return plan_fail(why, -1, "rows %d outside [1, max_rows=%d]", R, max_rows);
    // (strictly increasing from 0 to n_paths: every entry indexes pro; a path's rows are checked against R before row_t is written)
    for (int i = 0; i < M; ++i)
        if (tpo[i + 1] <= tpo[i]) return plan_fail(why, -1, "task %d has no paths", i);
    std::vector<int> path_task(n_paths), row_t(R), tro(M + 1);
    for (int i = 0; i < M; ++i) {
        tro[i] = pro[tpo[i]];
        for (int p = tpo[i]; p < tpo[i + 1]; ++p) {
            if (pro[p + 1] < pro[p] || pro[p + 1] > R) return plan_fail(why, -1, "path_row_offsets must be non-decreasing");
            path_task[p] = i;
            for (int r = pro[p]; r < pro[p + 1]; ++r) row_t[r] = r - pro[p];
        }
        if (pro[tpo[i + 1]] == tro[i]) return plan_fail(why, -1, "task %d has no rows", i);
    }
    tro[M] = R;
    // work tables: contiguous ranges of 16-row wave tiles, workgroups shared out over tasks in proportion to their tiles
    std::vector<int> tiles(M);
    long long total_tiles = 0;
    const int GR = 16;   // work granule = one wave tile (16 rows)
    for (int i = 0; i < M; ++i) { tiles[i] = (tro[i + 1] - tro[i] + GR - 1) / GR; total_tiles += tiles[i]; }
    std::vector<WorkItem> work[2];
    std::vector<int> two[2];
    for (int t = 0; t < 2; ++t) {
        // table 0: the cooperative pass kernels (one workgroup per CU: measured faster than two shorter ones, the parameter
        // staging and the end-of-kernel reduction amortise over twice the tiles); table 1: the sample-processing kernels
        int target = (t + 1) * n_cus;
        two[t].assign(M + 1, 0);
        // largest-remainder split: sum of workgroups <= target (one more would cost a whole second round on the chip),
        // every task gets at least one and at most one per tile
        std::vector<long long> nw(M), rem(M);
        long long used = 0;
        for (int i = 0; i < M; ++i) {
            const long long num = tiles[i] * (long long)target;
            nw[i] = num / total_tiles;
            rem[i] = num % total_tiles;
            if (nw[i] < 1) { nw[i] = 1; rem[i] = 0; }
            if (nw[i] > tiles[i]) { nw[i] = tiles[i]; rem[i] = 0; }
            used += nw[i];
        }
        while (used < target) {
            int best = -1;
            for (int i = 0; i < M; ++i)
                if (nw[i] < tiles[i] && rem[i] > 0 && (best < 0 || rem[i] > rem[best])) best = i;
            if (best < 0) break;
            nw[best] += 1;
            rem[best] = 0;
            used += 1;
        }
        for (int i = 0; i < M; ++i) {
            const long long w = nw[i];
            for (int g = 0; g < (int)w; ++g) {
                const int t0 = (int)((long long)tiles[i] * g / w), t1 = (int)((long long)tiles[i] * (g + 1) / w);
                WorkItem it;
                it.task = i;
                it.row_begin = tro[i] + t0 * GR;
                it.row_end = tro[i] + t1 * GR;
                if (it.row_end > tro[i + 1]) it.row_end = tro[i + 1];
                it.pad = 0;
                work[t].push_back(it);
            }
            two[t][i + 1] = (int)work[t].size();
        }
        if ((int)work[t].size() > max_work) return plan_fail(why, -5, "internal: work table overflow (%zu > %d)", work[t].size(), max_work);
    }
    // chain kernels: the NW waves of a workgroup walk a segment's tiles round-robin, so a task of n tiles costs
    // ceil(n / NW) rounds; the global list of rounds is cut into equal shares, one per CU; a share that straddles task
    // boundaries becomes one segment per task (walked one after the other).  Segments are generated in task order, so a
    // task's partial rows are the contiguous segment indices [slot_off[i], slot_off[i+1]).
    struct ChainTable { std::vector<ChainSeg> segs; std::vector<int> wg_off, slot_off; };
    ChainTable T;
    {
        const int NW = CHAIN_NW_HVP;
        std::vector<long long> rounds(M);
        long long total = 0;
        for (int i = 0; i < M; ++i) { rounds[i] = (tiles[i] + NW - 1) / NW; total += rounds[i]; }
        // A segment also costs its parameter staging and end reduction, about SEGC rounds' worth: workgroups are filled
        // up to a common cost limit (rounds + SEGC per segment, in quarter rounds), the smallest limit that needs no more
        // workgroups than there are CUs.
        const long long SEGC = 2;                  // quarter rounds per segment
        auto cut = [&](long long limit, bool emit) -> long long {
            long long nwg = 0, cost = 0;
            bool open = false;
            for (int i = 0; i < M; ++i) {
                long long done = 0;
                while (done < rounds[i]) {
                    long long room = open ? (limit - cost - SEGC) / 4 : 0;   // rounds of task i that still fit
                    if (!open || room < 1) {
                        if (open && emit) T.wg_off.push_back((int)T.segs.size());
                        ++nwg; open = true; cost = 0;
                        room = (limit - SEGC) / 4;
                        if (room < 1) room = 1;
                    }
                    const long long take = std::min(room, rounds[i] - done);
                    if (emit) {
                        ChainSeg sg;
                        sg.task = i;
                        sg.tile0 = (int)(done * NW);
                        sg.ntiles = (int)std::min<long long>(tiles[i], (done + take) * NW) - sg.tile0;
                        sg.pad = 0;
                        T.segs.push_back(sg);
                        T.slot_off[i + 1] = (int)T.segs.size();
                    }
                    done += take;
                    cost += 4 * take + SEGC;
                }
            }
            if (open && emit) T.wg_off.push_back((int)T.segs.size());
            return nwg;
        };
        long long lo = 4 + SEGC, hi = 4 * total + SEGC * M + 4;
        while (lo < hi) {
            const long long mid = (lo + hi) / 2;
            if (cut(mid, false) <= n_cus) hi = mid; else lo = mid + 1;
        }
        T.slot_off.assign(M + 1, 0);
        T.wg_off.assign(1, 0);
        cut(lo, true);
        for (int i = 0; i < M; ++i)
            if (T.slot_off[i + 1] < T.slot_off[i]) T.slot_off[i + 1] = T.slot_off[i];
        if ((int)T.segs.size() > max_work) return plan_fail(why, -5, "internal: segment table overflow (%zu > %d)", T.segs.size(), max_work);
    }
    out->pro.assign(pro, pro + n_paths + 1); out->tpo.assign(tpo, tpo + M + 1);
    out->path_task = std::move(path_task); out->row_t = std::move(row_t); out->tro = std::move(tro);
    out->wg_off = std::move(T.wg_off); out->slot_chain = std::move(T.slot_off);
    out->segs = std::move(T.segs);
    for (int t = 0; t < 2; ++t) { out->two[t] = std::move(two[t]); out->work[t] = std::move(work[t]); }
    return 0;
}

// ---- selections (promp_set_step_selection) ---------------------------------------------------------------------------------
// How many of a task's P paths a subsampling factor f in (0, 1] keeps: floor(f P), at least one.  The guard keeps products that
// are whole numbers on paper from landing just below them (0.29 * 100 = 28.999999999999996).
inline int selection_count(double f, int n_paths) {
    const int n = (int)std::floor(f * (double)n_paths + 1e-6);
    return n < 1 ? 1 : n > n_paths ? n_paths : n;
}
// A selection of a step's paths and the layout of the slab that holds copies of their rows in path order: what
// promp_upload_step would be given for the selected paths alone.
struct SelectionLayout {
    std::vector<int> idx;          // [n_sel] the selected paths, strictly increasing
    std::vector<int> tpo, pro;     // [tasks + 1] / [n_sel + 1] offsets of the compact slab
};
// Checks a selection against the step's layout (tpo [M + 1], pro [n_paths + 1], both well-formed) before anything is indexed by
// it: indices inside the step, strictly increasing, at least one path left in every task.  Nothing is written on refusal.
inline int build_selection(int M, int n_paths, const int32_t* tpo, const int32_t* pro, int n_sel, const int32_t* idx,
                           SelectionLayout* out, std::string* why) {
    if (n_sel < 0) return plan_fail(why, -1, "n_sel %d is negative", n_sel);
    if (n_sel < 1 || !idx) return plan_fail(why, -1, "an empty selection (n_sel = 0 or NULL clears the step's selection)");
    if (n_sel > n_paths) return plan_fail(why, -1, "selection of %d paths from a step of %d", n_sel, n_paths);
    for (int j = 0; j < n_sel; ++j) {
        if (idx[j] < 0 || idx[j] >= n_paths)
            return plan_fail(why, -1, "selection entry %d: path index %d out of range [0, %d)", j, idx[j], n_paths);
        if (j > 0 && idx[j] == idx[j - 1]) return plan_fail(why, -1, "selection entry %d repeats path %d", j, idx[j]);
        if (j > 0 && idx[j] < idx[j - 1])
            return plan_fail(why, -1, "selection is not sorted: entry %d (path %d) follows path %d", j, idx[j], idx[j - 1]);
    }
    SelectionLayout L;
    L.idx.assign(idx, idx + n_sel);
    L.tpo.assign(M + 1, 0);
    L.pro.assign(n_sel + 1, 0);
    int j = 0;
    for (int i = 0; i < M; ++i) {
        while (j < n_sel && idx[j] < tpo[i + 1]) {
            L.pro[j + 1] = L.pro[j] + (pro[idx[j] + 1] - pro[idx[j]]);
            ++j;
        }
        if (j == L.tpo[i]) return plan_fail(why, -1, "selection leaves task %d with no path", i);
        L.tpo[i + 1] = j;
    }
    *out = std::move(L);
    return 0;
}
// A selection as the table of the copy launch (k_scatter_partition): [n_paths][2], selected path q to slab 0 at the row lay.pro[q]
// of its compact slab, every other path to slab -1: nowhere.  The partition into one minibatch in which some paths are dropped.
inline std::vector<int> selection_copy_table(int n_paths, const SelectionLayout& lay) {
    std::vector<int> copy(2 * (size_t)n_paths, 0);
    for (int p = 0; p < n_paths; ++p) copy[2 * (size_t)p] = -1;
    for (size_t q = 0; q < lay.idx.size(); ++q) {
        copy[2 * (size_t)lay.idx[q]] = 0;
        copy[2 * (size_t)lay.idx[q] + 1] = lay.pro[q];
    }
    return copy;
}

// ---- partitions (promp_optimize_minibatch) -----------------------------------------------------------------------------------
// A step's paths dealt to B minibatches: per minibatch the selection of its paths and the tables of the compact slab that holds
// them -- what build_selection + build_step_tables give for {p : assign[p] = j} --, and the table of the one copy launch that
// fills all B slabs (k_scatter_partition).  The slabs lie one behind the other, [minibatch][task][path]: minibatch j's rows are
// [row_base[j], row_base[j + 1]) of the step's R rows.
struct PartitionLayout {
    std::vector<SelectionLayout> lay;      // [B]
    std::vector<StepTables> tables;        // [B]
    std::vector<int> row_base;             // [B + 1]
    std::vector<int> copy;                 // [n_paths][2]: the minibatch of a source path, the first of its destination rows
};
// tpo [M + 1], pro [n_paths + 1]: the step's offsets, well-formed; assign [n_paths] in [0, B).  Refuses B < 1, B above a task's
// path count, an entry outside [0, B) and a (minibatch, task) left without a path; nothing is written on refusal.
inline int build_partition(int n_cus, int max_work, int M, int n_paths, const int32_t* tpo, const int32_t* pro, int B,
                           const int32_t* assign, PartitionLayout* out, std::string* why) {
    if (B < 1) return plan_fail(why, -1, "num_minibatches %d is below 1", B);
    if (!assign) return plan_fail(why, -1, "the assignment is NULL");
    for (int i = 0; i < M; ++i)
        if (B > tpo[i + 1] - tpo[i])
            return plan_fail(why, -1, "num_minibatches %d exceeds the %d paths of task %d", B, tpo[i + 1] - tpo[i], i);
    for (int p = 0; p < n_paths; ++p)
        if (assign[p] < 0 || assign[p] >= B)
            return plan_fail(why, -1, "assignment entry %d: minibatch %d out of range [0, %d)", p, assign[p], B);
    std::vector<std::vector<int32_t>> idx(B);
    for (int i = 0; i < M; ++i) {
        std::vector<int> have(B, 0);
        for (int p = tpo[i]; p < tpo[i + 1]; ++p) have[assign[p]] += 1;
        for (int j = 0; j < B; ++j)
            if (!have[j]) return plan_fail(why, -1, "the assignment leaves minibatch %d without a path of task %d", j, i);
    }
    for (int p = 0; p < n_paths; ++p) idx[assign[p]].push_back(p);
    PartitionLayout L;
    L.lay.resize(B);
    L.tables.resize(B);
    L.row_base.assign(B + 1, 0);
    L.copy.assign(2 * (size_t)n_paths, 0);
    for (int j = 0; j < B; ++j) {
        const int n = (int)idx[j].size();
        if (const int rc = build_selection(M, n_paths, tpo, pro, n, idx[j].data(), &L.lay[j], why)) return rc;
        const SelectionLayout& s = L.lay[j];
        if (const int rc = build_step_tables(n_cus, max_work, s.pro[n], n, M, n, s.tpo.data(), s.pro.data(), &L.tables[j], why)) return rc;
        L.row_base[j + 1] = L.row_base[j] + s.pro[n];
        for (int q = 0; q < n; ++q) {
            L.copy[2 * (size_t)s.idx[q]] = j;
            L.copy[2 * (size_t)s.idx[q] + 1] = L.row_base[j] + s.pro[q];
        }
    }
    *out = std::move(L);
    return 0;
}

// ---- table blocks ------------------------------------------------------------------------------------------------------------
// Everything one copy launch and the passes on the B compact slabs it fills read of the layout, in ONE block of ints that a single
// copy sends: the copy table [paths][2] at 0, the slabs' shifts [B] (rows between a slab's place in its pool and its offset in the
// copy table), then per slab its pass tables tro | two | slot | wg_off | work | segs.  Every piece starts on a multiple of 64
// ints.  A selection's block is the same shape with B = 1.
struct TableBlock {
    size_t shift = 0, slab0 = 0, slab_stride = 0, total = 0;
    size_t tro = 0, two = 0, slot = 0, wg_off = 0, work = 0, segs = 0;      // inside a slab's part
    static size_t r64(size_t n) { return (n + 63) & ~(size_t)63; }
    TableBlock(int n_paths, int B, int M, int max_work) {
        static_assert(sizeof(WorkItem) == 4 * sizeof(int) && sizeof(ChainSeg) == 4 * sizeof(int), "tables are packed as ints");
        shift = r64(2 * (size_t)n_paths);
        slab0 = shift + r64(B);
        two = r64(M + 1); slot = 2 * r64(M + 1); wg_off = 3 * r64(M + 1);
        work = wg_off + r64((size_t)max_work + 1);
        segs = work + r64(4 * (size_t)max_work);
        slab_stride = segs + r64(4 * (size_t)max_work);
        total = slab0 + (size_t)B * slab_stride;
    }
    size_t slab(int j) const { return slab0 + (size_t)j * slab_stride; }
};
// one slab's pass tables into its part s [blk.slab_stride] of a block's image (t built for at most the block's max_work and M)
inline void pack_slab_tables(const TableBlock& blk, const StepTables& t, int* s) {
    memcpy(s + blk.tro, t.tro.data(), sizeof(int) * t.tro.size());
    memcpy(s + blk.two, t.two[0].data(), sizeof(int) * t.two[0].size());
    memcpy(s + blk.slot, t.slot_chain.data(), sizeof(int) * t.slot_chain.size());
    memcpy(s + blk.wg_off, t.wg_off.data(), sizeof(int) * t.wg_off.size());
    memcpy(s + blk.work, t.work[0].data(), sizeof(WorkItem) * t.work[0].size());
    memcpy(s + blk.segs, t.segs.data(), sizeof(ChainSeg) * t.segs.size());
}
// the block's image in dst [blk.total]: copy [paths][2], shifts [B], the pass tables of tables [B]
inline void pack_table_block(const TableBlock& blk, const std::vector<int>& copy, const std::vector<int>& shifts,
                             const StepTables* tables, int* dst) {
    memset(dst, 0, sizeof(int) * blk.total);
    memcpy(dst, copy.data(), sizeof(int) * copy.size());
    memcpy(dst + blk.shift, shifts.data(), sizeof(int) * shifts.size());
    for (size_t j = 0; j < shifts.size(); ++j) pack_slab_tables(blk, tables[j], dst + blk.slab((int)j));
}

// ---- outer step (promp_set_outer_optimizer) ----------------------------------------------------------------------------------
// What the general final-stage kernels (k_final_outer / k_mean_outer, promp_kernels_policy.h) take by value.  one_minus_b* are
// rounded on the host from the double difference, so that default arguments give the 0.1f and 0.001f of the plain kernels.
struct OuterOptArgs {
    int rule;                  // PROMP_OUTER_*
    float b1, one_minus_b1, b2, one_minus_b2, eps;      // Adam
    float mu;                  // Momentum
    int nesterov;
    float max_norm;            // > 0: clip the task-mean gradient by its global norm (split kernels only); 0: off
};
// The context's settings.  The betas are doubles: lr_t is computed in double, and the defaults are the double constants 0.9 and
// 0.999 -- a float argument that equals a default's float32 value means that default (outer_opt_plan), so that asking for the
// default by name changes no bit.
struct OuterOptPlan {
    int rule = PROMP_OUTER_ADAM;
    double b1 = 0.9, b2 = 0.999;
    float eps = 1e-8f;
    float mu = 0.f;
    int nesterov = 0;
    float max_norm = 0.f;
};
inline const char* outer_rule_name(int rule) {
    return rule == PROMP_OUTER_ADAM ? "adam" : rule == PROMP_OUTER_SGD ? "sgd" : rule == PROMP_OUTER_MOMENTUM ? "momentum" : nullptr;
}
// 'adam' | 'sgd' / 'gradient_descent' | 'momentum', or TF1's class names; -1: not a rule of this library (RMSProp and the rest)
inline int outer_rule_by_name(const char* name) {
    if (!name) return -1;
    const std::string n(name);
    if (n == "adam" || n == "AdamOptimizer") return PROMP_OUTER_ADAM;
    if (n == "sgd" || n == "gradient_descent" || n == "GradientDescentOptimizer") return PROMP_OUTER_SGD;
    if (n == "momentum" || n == "MomentumOptimizer") return PROMP_OUTER_MOMENTUM;
    return -1;
}
// Validates promp_set_outer_optimizer's arguments (args may be NULL: the rule's defaults) and writes the plan; nothing is written
// on refusal.  Only the arguments of the rule asked for are read.
inline int outer_opt_plan(int rule, const float* args, float max_grad_norm, OuterOptPlan* out, std::string* why) {
    if (!outer_rule_name(rule))
        return plan_fail(why, -1, "outer optimiser rule %d unknown (0 adam, 1 sgd, 2 momentum; RMSProp and others are not built)", rule);
    if (!(max_grad_norm >= 0.f) || !std::isfinite(max_grad_norm))
        return plan_fail(why, -1, "max_grad_norm %g must be finite and >= 0 (0: no clipping)", (double)max_grad_norm);
    OuterOptPlan p;
    p.rule = rule;
    p.max_norm = max_grad_norm;
    if (rule == PROMP_OUTER_ADAM && args) {
        if (!(args[0] >= 0.f && args[0] < 1.f)) return plan_fail(why, -1, "beta1 %g outside [0, 1)", (double)args[0]);
        if (!(args[1] >= 0.f && args[1] < 1.f)) return plan_fail(why, -1, "beta2 %g outside [0, 1)", (double)args[1]);
        if (!(args[2] > 0.f) || !std::isfinite(args[2])) return plan_fail(why, -1, "epsilon %g must be positive and finite", (double)args[2]);
        p.b1 = args[0] == 0.9f ? 0.9 : (double)args[0];
        p.b2 = args[1] == 0.999f ? 0.999 : (double)args[1];
        p.eps = args[2];
    }
    if (rule == PROMP_OUTER_MOMENTUM && args) {
        if (!(args[0] >= 0.f && args[0] < 1.f)) return plan_fail(why, -1, "momentum %g outside [0, 1)", (double)args[0]);
        if (args[1] != 0.f && args[1] != 1.f) return plan_fail(why, -1, "use_nesterov %g must be 0 or 1", (double)args[1]);
        p.mu = args[0];
        p.nesterov = args[1] != 0.f;
    }
    *out = p;
    return 0;
}
// (promp_get_outer_optimizer: the arguments in promp_set_outer_optimizer's layout)
inline void outer_opt_unplan(const OuterOptPlan& p, int* rule, float* args, float* max_grad_norm) {
    if (rule) *rule = p.rule;
    if (max_grad_norm) *max_grad_norm = p.max_norm;
    if (!args) return;
    args[0] = args[1] = args[2] = args[3] = 0.f;
    if (p.rule == PROMP_OUTER_ADAM) { args[0] = (float)p.b1; args[1] = (float)p.b2; args[2] = p.eps; }
    if (p.rule == PROMP_OUTER_MOMENTUM) { args[0] = p.mu; args[1] = (float)p.nesterov; }
}
inline bool outer_opt_is_default(const OuterOptPlan& p) {
    return p.rule == PROMP_OUTER_ADAM && p.b1 == 0.9 && p.b2 == 0.999 && p.eps == 1e-8f && p.max_norm == 0.f;
}
inline OuterOptArgs outer_opt_args(const OuterOptPlan& p) {
    OuterOptArgs o;
    o.rule = p.rule;
    o.b1 = (float)p.b1; o.one_minus_b1 = (float)(1.0 - p.b1);
    o.b2 = (float)p.b2; o.one_minus_b2 = (float)(1.0 - p.b2);
    o.eps = p.eps; o.mu = p.mu; o.nesterov = p.nesterov; o.max_norm = p.max_norm;
    return o;
}
// The learning rate a step's launch carries, t the step count INCLUDING this step: Adam's bias-corrected lr_t, in double; the
// call's own learning rate under the other rules.
inline float outer_lr_t(const OuterOptPlan& p, float lr, long long t) {
    if (p.rule != PROMP_OUTER_ADAM) return lr;
    const double td = (double)t;
    return (float)((double)lr * std::sqrt(1.0 - std::pow(p.b2, td)) / (1.0 - std::pow(p.b1, td)));
}
// Which kernels run the final stage of an evaluation.  Default settings: the plain instances (k_final_adam on one rank,
// k_reduce_final -> exchange -> k_mean_adam where the sums cross ranks: split_wanted), as in a library without the settings.
// Anything else, or PROMP_OUTER_GENERIC=1, on a STEPPING evaluation: the general family (k_final_outer / k_mean_outer).
// Clipping needs the norm before any entry is stepped: always the split route.  An evaluation that does not step has no use for
// a rule or a norm and stays on the plain instances.
struct FinalPlan {
    bool general;
    bool split;
};
inline FinalPlan final_stage_plan(const OuterOptPlan& p, const PlanSwitches& sw, bool stepping, bool split_wanted) {
    FinalPlan f;
    f.general = stepping && (sw.outer_generic || !outer_opt_is_default(p));
    f.split = split_wanted || (stepping && p.max_norm > 0.f);
    return f;
}
// The whole launch decision of a final stage over Theta = NP parameters and K inner steps: the plan above, whether the step
// sizes' Theta columns ride along (the *_ss instances), the floats of the exchange buffer -- [grad Theta | K + 2 scalars] and
// behind them the step-size gradient's Theta sums --, and every grid.  Reduce and fused launches: 64 columns per block, the fused
// one with one more block for the statistics; the mean launch: 256 threads per block, theta's entries, the statistics thread
// and the step sizes' entries.
struct FinalLaunch {
    bool general, split, sizes;
    size_t red_count;
    unsigned reduce_grid, mean_grid, fused_grid;
};
inline size_t final_red_count(int NP, int K, bool sizes) { return (size_t)(sizes ? 2 : 1) * NP + K + 2; }
inline FinalLaunch final_stage_launch(const FinalPlan& f, int NP, int K, bool sizes) {
    FinalLaunch L;
    L.general = f.general; L.split = f.split; L.sizes = sizes;
    L.red_count = final_red_count(NP, K, sizes);
    L.reduce_grid = (unsigned)((L.red_count + 63) / 64);
    L.mean_grid = (unsigned)(((size_t)(sizes ? 2 : 1) * NP + 1 + 255) / 256);
    L.fused_grid = L.reduce_grid + 1;
    return L;
}
