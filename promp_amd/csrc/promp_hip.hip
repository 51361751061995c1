// promp_hip.hip -- host side of libpromp_hip.so: context, device memory, launch sequences, C ABI.
// See include/promp_hip.h for the contract.  gfx950 only; built by __graft_entry__.build():
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC promp_hip.hip -lrccl -o libpromp_hip.so
#include "promp_plan.h"
#include "promp_kernels_chain.h"
#include "promp_kernels_pass.h"
#include "promp_kernels_policy.h"
#include "promp_kernels_policy_wide.h"
#include "promp_kernels_wide_bf16.h"
#include "promp_kernels_sample.h"
#include "promp_kernels_rollout.h"
#include "promp_kernels_generic.h"
#include "promp_kernels_generic_bf16.h"
#include "../../include/promp_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define PROMP_ARCH_NAME(prop) (prop).gcnArchName

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// a plan function (promp_plan.h) refused: its code, its message
int fail_plan(int code, const std::string& why) { return fail(code, "%s", why.c_str()); }

#define HIPCHECK(expr)                                                                            \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---- owners: every device allocation, page-locked host block, event and stream is released by the member that holds it ----
// Move-only; converts to the raw pointer / handle, so use sites read as if they held one.
template <class T, bool PINNED>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;                    // reserve(): elements held
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { (void)release(); }
    operator T*() const { return p; }
    hipError_t release() {
        T* q = p;
        p = nullptr; cap = 0;
        return !q ? hipSuccess : PINNED ? hipHostFree(q) : hipFree(q);
    }
    // n elements (at least one) in place of what it held; device memory arrives zero-filled
    int alloc(size_t n) {
        const size_t bytes = (n ? n : 1) * sizeof(T);
        HIPCHECK(release());
        if (PINNED) HIPCHECK(hipHostMalloc((void**)&p, bytes, hipHostMallocDefault));
        else {
            HIPCHECK(hipMalloc((void**)&p, bytes));
            HIPCHECK(hipMemset(p, 0, bytes));
        }
        return 0;
    }
    // room for n elements, contents not kept and not zeroed; a buffer that has to grow is replaced by one of slack * n
    int reserve(size_t n, size_t slack) {
        if (n <= cap) return 0;
        HIPCHECK(release());
        if (PINNED) HIPCHECK(hipHostMalloc((void**)&p, sizeof(T) * slack * n, hipHostMallocDefault));
        else HIPCHECK(hipMalloc((void**)&p, sizeof(T) * slack * n));
        cap = slack * n;
        return 0;
    }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;
template <class H, hipError_t (*DESTROY)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)DESTROY(h); }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// first line of an entry point that takes nothing but the context
#define NEED_CTX(c) \
    if (!(c)) return fail(-1, "ctx is NULL")

// What a policy pass (launch_pass, PassReq) reads of the rows it walks, stated once: a sampling step's own arrays (StepData::ps,
// bound by alloc_step) or a compact slab that holds copies of some of a step's paths (a selection's, a minibatch's: bound by
// scatter_slabs).  The arrays and tables are views -- their owner outlives every use of the slab --; the primal cache is the
// slab's own.  Its address is its identity (promp_ctx::wbp).
struct PassSlab {
    const float *obs = nullptr, *act = nullptr, *adv = nullptr, *old_mean = nullptr, *old_ls = nullptr;
    unsigned* obs_absmax = nullptr;    // [tasks]: bits of the largest |observation| of each task's rows (the FP16 split's scale)
    const int *task_row_offsets = nullptr, *task_wg_offsets = nullptr;   // [tasks + 1] each; the work items of a task
    const int *chain_slot_offsets = nullptr, *chain_wg_offsets = nullptr;
    const WorkItem* work = nullptr;    // one workgroup per CU (cooperative and layer-by-layer passes)
    const ChainSeg* chain_segs = nullptr;
    int n_rows = 0, n_work = 0, n_chain_wg = 0;
    int ls_per_row = 0;
    bool has_policy = false, has_adv = false;
    bool obs_range_valid = false;      // false from whatever writes obs until obs_absmax holds its range (enqueue_obs_range, the copy launch)
    unsigned long long data_version = 0;
    DevBuf<float> hcache;              // primal cache (promp_kernels_chain.h: chain_cache_row), allocated on first use ...
    size_t cache_rows = 0;             // ... for this many rows (a compact slab that outgrows it releases the cache)
    unsigned long long cache_tag = 0;  // identity of the primal cache's contents (every storing pass draws a new one)
};

struct StepData {
    int n_paths = 0, n_rows = 0;
    int n_work[2] = {0, 0};            // [0]: one workgroup per CU (wide passes, gram, fit), [1]: two per CU (k_normalize)
    int rollout_B = 0, rollout_T = 0;  // environments per task / horizon of a device-side rollout in progress (promp_begin_rollout)
    bool rollout_ragged = false;       // promp_begin_collection: rows go to the staging area, rollout_T = its capacity in vectorised steps
    // promp_policy_step_dev / promp_file_step_dev since the last promp_begin_rollout / promp_begin_collection: policy steps
    // 0 .. dev_policy_done - 1 have been taken, steps 0 .. dev_filed - 1 filed (host-side counters: every refusal precedes a launch)
    int dev_policy_done = 0, dev_filed = 0;
    int n_chain_wg = 0;                // workgroups of the register-chained kernels k_pass / k_chain_hvp (segment table)
    bool has_policy = false, processed = false, has_adv = false;
    unsigned long long data_version = 0;   // bumped by every entry point that may change what the policy passes read from this step
    int ls_per_row = 0;
    int feat_dim = 0;
    PassSlab ps;                       // the step as the policy passes see it: reach it through pass_slab()
    DevBuf<float> obs, act, rew, old_mean, old_ls;
    DevBuf<unsigned> obs_absmax;       // [tasks]: ps.obs_absmax (k_obs_range)
    DevBuf<double> rew64;              // promp_set_rewards_f64 (allocated on first use); valid while has_rew64
    // DiCE (promp_set_dice_rewards; allocated on first use): per-row adjusted rewards, row tangents of the R-operator pass,
    // coupling weights, scan scratch
    DevBuf<float> dice_rw, dice_c, dice_u;
    DevBuf<double> dice_tmp;
    bool has_dice = false;
    // promp_process_samples_dice (allocated on its first use): the normalised adjusted rewards and GAE advantages in float64,
    // the advantages as slab weights, the tasks' pad values [2][tasks], the reward baseline's coefficients (coeffs holds the
    // return baseline's after such a call), the per-path sums [3][paths]
    DevBuf<double> dice_x64, dice_adv64, dice_pad, dice_coeffs, dice_path;
    DevBuf<float> dice_vpg32;
    bool dice_processed = false, has_dice_vpg = false;
    int dice_feat_dim = 0, dice_ret_feat_dim = 0;
    bool has_rew64 = false;
    DevBuf<float> ret32, adv32;
    DevBuf<double> ret64, adv64;
    DevBuf<int> path_row_offsets, path_task, row_t;
    DevBuf<int> task_row_offsets, task_path_offsets;
    DevBuf<int> task_wg_offsets[2];
    DevBuf<ChainSeg> chain_segs;                             // segment table of k_pass / k_chain_hvp
    DevBuf<int> chain_wg_offsets;                            // [workgroups+1]
    DevBuf<int> chain_slot_offsets;                          // [tasks+1]: partial rows (= segments) of each task
    DevBuf<double> path_ret0, path_undisc, path_rsq, path_mom;
    DevBuf<double> coeffs;
    DevBuf<WorkItem> work[2];
    // second-stream sample processing (promp_process_samples of steps >= 1, see stage_a_stream):
    Event ev_use;                      // main stream: the last enqueued work that reads or writes this step's slabs
    Event ev_done;                     // side stream: the step's processed outputs are complete
    bool use_set = false, side_pending = false, dirty = false;
    // staged uploads (promp_stage_step / promp_commit_step): the slab set is written by the copy stream
    Event ev_ready;                    // copy stream: every array of this slab set has arrived
    bool ready_set = false, wait_ready_main = false, wait_ready_side = false, staged = false;
    std::shared_ptr<void> host_tables; // host-side sources of the asynchronous table copies, alive until the next staging
    std::vector<int> lay_tpo, lay_pro; // the offsets the set's device-side tables were built from (set_step_layout)
};

// k_pass instances: (hidden_0 / 16, hidden_1 / 16)
#define PROMP_PASS_ALL(X) X(2, 2) X(2, 4) X(4, 2) X(4, 4)
#define PROMP_WB_ALL(X) X(1, 4, 2) X(2, 7, 4) X(3, 8, 4)
#define PROMP_CHAIN_ALL(X) X(2, 2, 2) X(2, 2, 5) X(2, 2, 8) X(2, 4, 2) X(2, 4, 5) X(2, 4, 8) X(4, 2, 2) X(4, 2, 5) X(4, 2, 8) X(4, 4, 2) X(4, 4, 5) X(4, 4, 8)
// k_wide_* instances: (hidden width, observation blocks of 16)
#define PROMP_WIDE_ALL(X) X(128, 2) X(128, 4) X(128, 8) X(64, 2) X(64, 4) X(64, 8)

// One policy pass (launch_pass): the defaults are a first-order pass with the plain per-task reduction
struct PassReq {
    bool hvp = false;                  // R-operator pass along the direction in c->vbuf
    const float* theta = nullptr;      // parameters: one row per task at theta_stride (0: one row shared by every task)
    long long theta_stride = 0;
    int loss_kind = LOSS_RATIO;
    float clip_eps = 0.f;
    int clip_ls = 0;                   // clip log_std at log(min_std)
    float klw = 0.f;                   // weight of the KL term
    bool fwd_only = false;             // loss and KL only, no gradient
    int red_mode = RED_PLAIN;          // k_reduce_task (promp_kernels_chain.h): RED_STEP / RED_OUTER / RED_HVP / RED_PLAIN / RED_SCAL
    const float* cur = nullptr;        // RED_STEP: next = cur - step sizes * gradient
    long long cur_stride = 0;
    float* next = nullptr;
    float* scal = nullptr;             // per-task loss and KL (nullptr: c->scal_tmp)
    int cache = 0;                     // primal cache: 0 none, 1 the gradient pass fills it, 2 the R-operator pass reads it
    const float* adv = nullptr;        // per-row weights instead of the step's advantages (DiCE coupling pass)
    float* row_tan = nullptr;          // R-operator pass: where the rows' log-likelihood tangents go (DiCE)
    float* next2 = nullptr;            // RED_STEP: second destinations of next and scal (see adapt0)
    float* scal2 = nullptr;
    float* ginner = nullptr;           // RED_STEP: where the summed gradient itself goes (trainable step sizes)
};

// promp_constraint_hvp: what its primal caches (one per step) were filled at; the products of one conjugate-gradient solve run
// at the same parameters on the same slabs, so the 2K + 1 R-operator passes of every product after the first read them back
struct ChvpRec {
    bool valid = false;
    unsigned long long theta_version = 0, sizes_version = 0, data_version[PROMP_ETA_MAX + 1] = {}, tag[PROMP_ETA_MAX + 1] = {};
    int inner_kind = 0;
    float min_log_std = 0.f;
};

// The device side of a step's compact slabs: one pooled allocation per row array (every slab starts on a multiple of 64 rows),
// the observation ranges [slabs][tasks], and the table block (promp_plan.h: TableBlock) that one copy fills.  The slabs
// themselves are PassSlabs whose pointers lead into these (scatter_slabs).
struct SlabPool {
    DevBuf<float> obs, act, adv, mean, ls;
    DevBuf<unsigned> absmax;
    DevBuf<int> tables;
    size_t cap_rows = 0, cap_tables = 0, cap_absmax = 0;
    bool ls_rows = false;
};

// promp_set_step_selection: the paths of a step that the subsampled constraint products keep.  The compact slab that holds copies
// of their rows (promp_ctx::sub) is filled by the first evaluation that needs it and again whenever the step's data has moved.
struct Selection {
    bool on = false;
    SelectionLayout lay;
    StepTables tables;                 // the compact slab's tables, as build_step_tables lays out an upload of the selected paths
    std::vector<int> image;            // the table block (one slab; the copy table sends the other paths nowhere)
    SlabPool pool;
    bool gathered = false;
    unsigned long long gathered_version = 0;   // the step's data_version the copies were taken at
};

// What an evaluation of the meta-objective or of the constraint product walks and leaves behind: the whole batch with the
// context's chain of adapted parameters, or compact slabs (the selections', a minibatch's) with a chain, inner scalars and cache
// record of their own (what promp_inner_adapt and the last full-batch product left behind stays valid under a subsampled solve)
struct EvalSet {
    PassSlab* slab[PROMP_ETA_MAX + 1];
    StepData* full;                    // the steps that own the slabs (stream joins, use marks, DiCE rows); nullptr: compact slabs
    float* chain;
    float* scal_inner;
    ChvpRec* chvp;
};

struct ProfSlot {
    std::vector<Event> ev;       // start/stop pairs
    size_t used = 0;
    double total_ms = 0.0;
    long long launches = 0, rows = 0;
};

}  // namespace

struct promp_ctx {
    promp_dims d;
    int device = 0, n_cus = 256, clock_mhz = 0;
    char dev_name[256];
    int NP = 0, Dmax = 0, coeff_stride = 0, max_work = 0, partial_stride = 0, gram_stride = 0;
    promp_dims du;                       // the caller's dims (d holds the instantiated, possibly zero-padded hidden widths)
    int NPu = 0;                         // parameter count in the caller's layout
    bool padded = false;
    // (members are released in reverse order of declaration: the streams outlive every buffer and event below)
    Stream stream;
    Stream side;                         // sample processing of steps >= 1 runs here, under the main stream's step-0 work
    Stream copy;                         // promp_stage_step: host -> device copies of the NEXT batch, under the current one's compute
    std::vector<StepData> back;          // the slab sets being staged (swapped with `steps` entries by promp_commit_step)
    bool overlap = true;
    DevBuf<double> gram_partials_side, fit_scratch_side;
    std::vector<StepData> steps;
    DevBuf<float> theta, step_sizes, adam_m, adam_v;
    long long adam_t = 0;
    OuterOptPlan outer;                  // promp_set_outer_optimizer: the rule of every step, its arguments, the clip
    DevBuf<float> grad_norm;             // [1] the unclipped global norm k_mean_outer left (promp_get_grad_norm); allocated with the first clip
    bool norm_valid = false;             // a clipped step has been enqueued since clipping was switched on
    DevBuf<float> theta_tasks, chain, lam, vbuf;
    bool tasks_shared = false;           // switch_to_pre_update: every task's parameters ARE theta; theta_tasks is written when somebody reads it
    DevBuf<float> wbuf;                  // promp_constraint_hvp: [tasks][Theta], allocated on first use
    DevBuf<float> partials, scal_inner, scal_outer, scal_tmp;
    DevBuf<float> red, grad_mean, stats;
    float eta_last[PROMP_ETA_MAX] = {};
    DevBuf<double> gram_partials, red64;
    DevBuf<char> rollout_buf;            // goals, start states and noise of a device rollout (bytes)
    DevBuf<float> stage_rows;            // promp_begin_collection: staging rows [steps][tasks * B] of observations | actions | means
    DevBuf<double> point_norm;           // promp_point_norm_set: the normalize wrapper's running moments [n_envs][2 state_dim + 2]
    int point_norm_envs = 0, point_norm_dim = 0;   // what it was set for (0: not set)
    DevBuf<double> point_norm_stage;     // promp_collect_point_family_norm: the moments behind every step [max_steps][2 state_dim + 2][n_envs]
    DevBuf<double> fit_scratch;          // k_fit_wide: [tasks][2][(D+1)^2] when the matrices do not fit in LDS
    size_t smem_fwd = 0, smem_hvp = 0;
    PlanSwitches sw;                     // the PROMP_* switches, as promp_ctx_create found them
    PassFamily family = PassFamily::Chain;
    int wb_cls = 0;                      // CoopSplit: the observation class 1..3 (pass_family)
    size_t smem_wb_fwd = 0, smem_wb_bwd = 0, smem_wb_hvp = 0;
    DevBuf<unsigned> wb_planes, wb_vplanes;                 // [tasks][wb_planes_words]: k_wb_planes' output for theta / the direction
    // The planes of the META-parameters (theta itself, stride 0) have their own block: an epoch passes over step 0 at theta twice --
    // the inner gradient pass and, two passes later, the R-operator pass -- and the second finds the first one's planes (same
    // parameters, same slab, same observation scales): one k_wb_planes launch less per epoch.
    DevBuf<unsigned> wb_planes_meta;
    DevBuf<float> cg_buf;                // promp_cg_solve: x, r, d, (H + reg I) d, the gradient ahead, theta0 [+ the gradient at theta0]
    DevBuf<double> cg_scal;              // [4] r.r, d.Hd, converged, x.Hx
    struct { bool valid = false; unsigned long long theta_version = 0, data_version = 0, sizes_version = 0; const void* step = nullptr; } wbp;
    DevBuf<unsigned> vdir_absmax;        // [tasks]: k_vec_absmax's output for the direction (FP16 split)
    // layer-by-layer kernels (promp_kernels_generic.h) for every other shape: layer table, and one set of activation / tangent /
    // cotangent buffers for the whole context (the passes of a context run one after another on its stream)
    int gramt_map_nblk = -1;             // the block count c->gramt_map was balanced for
    GramtMap gramt_map;                  // one-slice k_gram_tiled launches: wave -> rectangle
    bool gen_bf16 = true;                // Layered: the GEMMs on the BF16 matrix pipe (promp_kernels_generic_bf16.h); PROMP_GEN_FP32=1: the exact-FP32 kernels (A/B runs)
    DevBuf<unsigned short> gb_wplanes, gb_vplanes;                 // [tasks][gb_plane_stride]: k_gb_planes' output for theta / minus the direction
    long long gb_plane_stride = 0;
    int gb_pf_off[GEN_MAX_LIN] = {}, gb_pb_off[GEN_MAX_LIN] = {};
    int n_lin = 0, g_maxw = 0;
    GenLin lin[GEN_MAX_LIN];
    DevBuf<float> g_act[GEN_MAX_LIN], g_ract[GEN_MAX_LIN], g_mu, g_rmu, g_dz[2], g_qz[2];
    DevBuf<unsigned long long> dbg;      // cycle stamps (developer tooling, tools/phase_timing.py)
    bool dbg_enabled = false;
    DevBuf<int> task_counters;           // [tasks] arrival counters of the chain kernels' fused reductions (zero between launches)
    DevBuf<int> split_events;            // [2] see PassArgs::split_events
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    float min_log_std = -13.815510558f;  // log(1e-6): GaussianMLPPolicy's default min_std
    bool learn_std = true;               // false: log_std is neither adapted (step size 0) nor trained (no Adam update)
    int fuse_min_tasks = 1 << 30;        // k_chain_hvp sums a task's partial rows in-launch from this many local tasks on (default: never)
    int stats_slot = 0;                  // promp_optimize parks the first epoch's statistics in slot 1 (loss_before)
    int primal_cache = -1;               // promp_set_primal_cache: 1 on, 0 off, -1 default (on: primal_cache_on)
    // promp_inner_adapt(step 0) from the meta-parameters evaluates exactly what the first epoch of the following optimisation
    // evaluates first (the inner pass at theta on step 0's slab): it leaves theta', the inner scalars and the primal cache
    // where that epoch expects them, and the epoch skips its pass while nothing it depends on has changed (reuse_adapt).
    unsigned long long version_counter = 0, theta_version = 0, sizes_version = 0;
    unsigned long long cache_counter = 0;   // tags of primal-cache fills: their own counter (whether a rank fills a cache depends on
                                            // its shard; promp_state_version must move alike on every rank)
    unsigned long long opt_theta_version = 0;   // theta_version when promp_optimize_begin returned (promp_optimize_end: ls_min)
    struct { bool valid = false; unsigned long long theta_version = 0, data_version = 0, sizes_version = 0; int inner_kind = 0; bool cached = false; float min_log_std = 0.f; bool learn_std = true; } adapt0;
    bool reuse_adapt = true;             // promp_set_reuse_adapt
    bool ls_known = false;               // ls_min is the smallest log_std entry of the current theta
    float ls_min = 0.f;
    ChvpRec chvp;
    // subsampled constraint products (promp_set_step_selection): per step the selection and its compact slab; the evaluations on
    // them keep their own chain, inner scalars and cache record (EvalSet), all allocated with the first selection
    std::vector<Selection> sel;
    std::vector<PassSlab> sub;
    DevBuf<float> sel_chain, sel_scal_inner;
    ChvpRec chvp_sel;
    bool use_sel = false;                // promp_use_selection: promp_meta_grad (outer kind KL) and promp_constraint_hvp run on the selections
    // minibatched Adam epochs (promp_optimize_minibatch): per step the pooled copies and the B slabs [steps][B]; the
    // evaluations on them keep a chain, inner scalars and a cache record of their own, like the selections'
    std::vector<SlabPool> mb_pool;
    std::vector<std::vector<PassSlab>> mb;
    DevBuf<float> mb_chain, mb_scal_inner;
    ChvpRec chvp_mb;
    PinBuf<int> mb_stage;                // page-locked sources of every (epoch, step) table copy of the pending optimisation
    bool mb_enqueued = false;            // copies out of mb_stage may still be on the stream (until promp_optimize_end)
    long long chvp_cached_passes = 0;          // R-operator passes of promp_constraint_hvp that read a primal cache (tests, tools)
    long long adapt_passes_skipped = 0;
    bool force_split = false;            // take the multi-rank launch sequence (reduce / all-reduce / Adam) on one rank too
    bool fixed_order = false;            // exchange = ncclAllGather + sum in rank order (bitwise-identical replicas) instead of ncclAllReduce
    DevBuf<float> gather;                // [nranks][Theta + K + 2]: every rank's sums side by side (fixed_order)
    bool prof = false;
    ProfSlot prof_slots[PROMP_KERNEL_COUNT];
    PinBuf<float> stats_host;            // pinned: promp_optimize_begin parks both statistics slots here (async copy)
    PinBuf<double> small_host;           // pinned: promp_download_processed gathers the per-path sums and coefficients here
    PinBuf<unsigned> stats_seq_host;     // pinned: sequence number the last launch of an optimisation writes behind the statistics
    unsigned stats_seq = 0;              // the number the pending optimisation will write
    bool publish_next = false;           // enqueue_meta: this launch is the one that publishes
    bool opt_pending = false;
    int opt_epochs = 0;
    DevBuf<float> fwd_buf;               // staging for promp_policy_forward
    // promp_set_train_step_sizes (promp_kernels_step_sizes.h), all allocated when the flag is first switched on: the inner
    // gradients g_k [K][tasks][Theta], the per-task step-size gradients [tasks][Theta], their task mean, alpha's Adam slots
    bool train_sizes = false;
    bool red_has_sizes = false;          // red's last Theta columns hold the step-size gradient's sums (promp_adam_step needs them)
    DevBuf<float> ginner, galpha, ss_grad, ss_m, ss_v;
    // environments on the device (the promp_*_dev rollout entry points).  What has to survive between the calls of one collection
    // has storage of its own -- rollout_buf is re-reserved by the other rollout calls --, reserved by the filing of step 0:
    // the staged rewards [max_steps][n_envs]; one integer block: end_len [max_steps][n_envs], ep_len [n_envs], step sums [max_steps],
    // task counts [tasks], task_path_offsets [tasks + 1], path_env / path_start / path_len [max_paths] each; k_collect_stop's record.
    DevBuf<float> dev_rew_stage;
    DevBuf<int> dev_tables;
    DevBuf<long long> dev_stop;
    // ordering against the caller's stream (producer_enter / producer_leave), created with the first such call, timing disabled
    Event ev_producer, ev_consumer;
};

namespace {

// lets each kernel take up to `bytes` of dynamic LDS
template <class... Kernels>
int allow_lds(int bytes, Kernels... kernels) {
    for (const void* k : {(const void*)kernels...}) HIPCHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

// ---- second stream for sample processing -------------------------------------------------------
// process_samples of a step >= 1 has no data dependence on the main stream's step-0 work (process_samples(0), _adapt):
// it is enqueued on c->side behind the last main-stream work that touched the step's slabs (ev_use), and the main stream
// picks the results up (ev_done) in front of the first launch that reads them.
//
// Event records are not free on the queue (a few microseconds of bubble each), so the uses are marked lazily: an entry
// point that touches a step only sets S.dirty on exit; the event is recorded when the next entry point that does NOT
// touch the step is about to enqueue (settle_others) -- in the training loop that is once per iteration, in front of
// process_samples(0).  A step still dirty when its processing goes to the side stream is marked on the spot, which
// orders it behind everything enqueued so far: always correct, merely no overlap.
int join_side(promp_ctx* c, StepData& S) {
    if (S.wait_ready_main) {           // slabs staged by the copy stream
        HIPCHECK(hipStreamWaitEvent(c->stream, S.ev_ready, 0));
        S.wait_ready_main = false;
    }
    if (!S.side_pending) return 0;
    HIPCHECK(hipStreamWaitEvent(c->stream, S.ev_done, 0));
    S.side_pending = false;
    return 0;
}
int mark_use(promp_ctx* c, StepData& S) {
    if (!S.dirty || !S.ev_use) return 0;
    HIPCHECK(hipEventRecord(S.ev_use, c->stream));
    S.use_set = true;
    S.dirty = false;
    return 0;
}
int settle_others(promp_ctx* c, const StepData* touched) {
    if (!c->overlap && c->back.empty()) return 0;
    for (auto& S : c->steps)
        if (&S != touched && mark_use(c, S)) return -2;
    for (auto& S : c->back)
        if (&S != touched && mark_use(c, S)) return -2;
    return 0;
}
// The prologue of an entry point that works on one step: the context and step checks, then open(): the join with the step's
// pending side-stream / copy-stream work, the other steps' use marks, and the check that the step holds data.  rc is what the
// entry point returns if any of it failed.  An entry point with checks of its own between the two halves calls open() itself.
struct StepScope {
    promp_ctx* c;
    int step;
    StepData* s = nullptr;
    int rc = 0;
    bool opened = false;
    StepScope(promp_ctx* c_, int step_) : c(c_), step(step_) {
        if (!c) rc = fail(-1, "ctx is NULL");
        else if (step < 0 || step > c->d.num_inner_steps) rc = fail(-1, "step %d out of range", step);
        else s = &c->steps[step];
    }
    StepScope(promp_ctx* c_, int step, bool writes, bool needs_data) : StepScope(c_, step) {
        if (!rc) open(writes, needs_data);
    }
    // writes: the entry point may change what a policy pass reads from the step (slabs, advantages, layout); pure readers say so
    int open(bool writes, bool needs_data) {
        opened = true;
        rc = join_side(c, *s) | settle_others(c, s);
        if (writes) s->data_version = ++c->version_counter;
        if (!rc && needs_data && s->n_rows == 0) rc = fail(-3, "step %d has no data", step);
        return rc;
    }
    ~StepScope() { if (opened) s->dirty = true; }
    StepData& S() const { return *s; }
};

// what the layer-by-layer kernels read as GenArgs.act_kind: the hidden nonlinearity's code in the low byte, the output
// nonlinearity's (mlp.py:53-60, 114-117; none = identity) above it
static int gen_act_kinds(const promp_dims* d) {
    const int out = d->hidden_act >> PROMP_OUT_ACT_SHIFT;
    const int ok = out == PROMP_OUT_ACT_TANH ? GEN_ACT_TANH : out == PROMP_OUT_ACT_RELU ? GEN_ACT_RELU : GEN_ACT_IDENTITY;
    return (d->hidden_act & 0xff) | (ok << 8);
}

// ---- profiling helpers -------------------------------------------------------------------------
int prof_begin(promp_ctx* c, int id, long long rows) {
    if (!c->prof) return 0;
    ProfSlot& s = c->prof_slots[id];
    if (s.used + 2 > s.ev.size()) {
        Event a, b;
        HIPCHECK(hipEventCreate(&a.h));
        HIPCHECK(hipEventCreate(&b.h));
        s.ev.push_back(std::move(a));
        s.ev.push_back(std::move(b));
    }
    HIPCHECK(hipEventRecord(s.ev[s.used], c->stream));
    s.rows += rows;
    return 0;
}
int prof_end(promp_ctx* c, int id) {
    if (!c->prof) return 0;
    ProfSlot& s = c->prof_slots[id];
    HIPCHECK(hipEventRecord(s.ev[s.used + 1], c->stream));
    s.used += 2;
    s.launches += 1;
    return 0;
}
int prof_collect(promp_ctx* c) {
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int id = 0; id < PROMP_KERNEL_COUNT; ++id) {
        ProfSlot& s = c->prof_slots[id];
        for (size_t i = 0; i + 1 < s.used; i += 2) {
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, s.ev[i], s.ev[i + 1]));
            s.total_ms += ms;
        }
        s.used = 0;
    }
    return 0;
}

// ---- launches ----------------------------------------------------------------------------------
// One layer's GEMM (k_gen_linear's MODE: GEN_FWD / GEN_BWD, the R-operator pass's GEN_FWD_T / GEN_BWD_T) or weight gradient
// (NT = 1, 2 with the tangents): on the BF16 matrix pipe, or the exact-FP32 kernels when PROMP_GEN_FP32=1 cleared gen_bf16.
template <int MODE, int NBW>
void gen_linear(promp_ctx* c, dim3 grid, const GenArgs& g, int li, int pp) {
    const int nt = (MODE == GEN_FWD_T || MODE == GEN_BWD_T) ? 2 : 1;
    if (c->gen_bf16) { auto k = k_gb_linear<MODE, NBW>; PROMP_LAUNCH(k, grid, 256, gb_smem(nt, NBW), c->stream, g, li, pp); }
    else { auto k = k_gen_linear<MODE, NBW>; PROMP_LAUNCH(k, grid, 256, gen_linear_smem(MODE, NBW), c->stream, g, li, pp); }
}
template <int NT, int NBW>
void gen_wgrad(promp_ctx* c, const PassSlab& S, const GenArgs& g, int li, int pp) {
    if (c->gen_bf16) {
        auto k = k_gb_wgrad<NT, NBW>;
        PROMP_LAUNCH(k, dim3(S.n_work * Ly_K_slabs(c->lin[li].K)), 256, gb_smem(NT, NBW), c->stream, g, li, pp);
    } else {      // one slab of 64 input units per workgroup
        auto k = k_gen_wgrad<NT, NBW>;
        PROMP_LAUNCH(k, dim3(S.n_work, (c->lin[li].K + GEN_KC - 1) / GEN_KC), 256, gen_wgrad_smem(NT, c->lin[li].N), c->stream, g, li, pp);
    }
}
// A pass on the layer-by-layer kernels (promp_kernels_generic.h): forward chain, loss level, then per layer (output first) the
// weight gradient and the cotangent of the layer below.  One workgroup per entry of work table 0 in every launch; the partial
// rows are the cooperative kernels' (one per work item, summed by k_reduce_task).
#define PROMP_GEN_NBW(nbw, ...) \
    switch (nbw) { case 1: { constexpr int NBW = 1; __VA_ARGS__ } break; case 2: { constexpr int NBW = 2; __VA_ARGS__ } break; \
                   case 3: { constexpr int NBW = 3; __VA_ARGS__ } break; default: { constexpr int NBW = 4; __VA_ARGS__ } break; }
// the context's layer table into the arguments of a layer-by-layer kernel
template <class Args>
void copy_layers(Args& dst, const promp_ctx* c) {
    dst.n_lin = c->n_lin;
    for (int l = 0; l < c->n_lin; ++l) dst.lin[l] = c->lin[l];
}
int launch_pass_generic(promp_ctx* c, PassSlab& S, const PassArgs& a, bool hvp, bool fwd_only) {
    GenArgs g;
    memset(&g, 0, sizeof g);
    g.work = a.work; g.task_row_offsets = a.task_row_offsets;
    copy_layers(g, c);
    g.O = a.O; g.A = a.A; g.NP = c->NP; g.act_kind = gen_act_kinds(&c->d);
    g.theta = a.theta; g.theta_task_stride = a.theta_task_stride; g.vdir = a.vdir;
    g.act[0] = a.obs;
    for (int l = 1; l < c->n_lin; ++l) { g.act[l] = c->g_act[l]; g.out_act[l] = c->g_act[l]; g.ract[l] = c->g_ract[l]; }
    g.mu = c->g_mu; g.rmu = c->g_rmu;
    g.dz[0] = c->g_dz[0]; g.dz[1] = c->g_dz[1]; g.qz[0] = c->g_qz[0]; g.qz[1] = c->g_qz[1];
    g.actions = a.act; g.adv = a.adv; g.old_mean = a.old_mean; g.old_log_std = a.old_log_std; g.ls_per_row = a.ls_per_row;
    g.partials = a.partials; g.partial_stride = a.partial_stride;
    g.loss_kind = a.loss_kind; g.clip_eps = a.clip_eps; g.clip_log_std = a.clip_log_std; g.min_log_std = a.min_log_std;
    g.kl_weight = a.kl_weight; g.row_tan = a.row_tan;
    const dim3 grid(S.n_work);
    // k_gen_linear / k_gb_linear: the 64-row rounds of a work item (about one CU's share of the rows) dealt to GEN_SPLIT workgroups
    const dim3 lgrid(S.n_work, GEN_SPLIT);
    hipStream_t st = c->stream;
    if (c->gen_bf16) {
        // the parameters' (and minus the direction's) kernels as BF16 planes, both orientations, in the GEMMs' chunk order
        GbPlaneArgs pa;
        memset(&pa, 0, sizeof pa);
        pa.n_lin = c->n_lin;
        int most = 0;
        for (int l = 0; l < c->n_lin; ++l) {
            pa.lin[l] = c->lin[l]; pa.pf_off[l] = c->gb_pf_off[l]; pa.pb_off[l] = c->gb_pb_off[l];
            g.pf_off[l] = c->gb_pf_off[l]; g.pb_off[l] = c->gb_pb_off[l];
            const int oct = (int)(gb_f_elems(c->lin[l].K, c->lin[l].N) / 24);
            most = oct > most ? oct : most;
        }
        const int gx = (most + 255) / 256 < 16 ? (most + 255) / 256 : 16;
        pa.src = a.theta; pa.src_task_stride = a.theta_task_stride; pa.dst = c->gb_wplanes;
        pa.dst_task_stride = a.theta_task_stride ? c->gb_plane_stride : 0; pa.sign = 1.f;
        PROMP_LAUNCH(k_gb_planes, dim3(gx, 2 * c->n_lin, a.theta_task_stride ? c->d.n_tasks : 1), 256, 0, st, pa);
        g.wplanes = c->gb_wplanes; g.wplane_stride = pa.dst_task_stride;
        if (hvp) {
            pa.src = a.vdir; pa.src_task_stride = c->NP; pa.dst = c->gb_vplanes; pa.dst_task_stride = c->gb_plane_stride; pa.sign = -1.f;
            PROMP_LAUNCH(k_gb_planes, dim3(gx, 2 * c->n_lin, c->d.n_tasks), 256, 0, st, pa);
            g.vplanes = c->gb_vplanes; g.vplane_stride = c->gb_plane_stride;
        }
    }
    for (int li = 0; li < c->n_lin; ++li) {
        const int nbw = (c->lin[li].N + 63) / 64;
        PROMP_GEN_NBW(nbw, if (hvp) gen_linear<GEN_FWD_T, NBW>(c, lgrid, g, li, 0); else gen_linear<GEN_FWD, NBW>(c, lgrid, g, li, 0);)
    }
    if (hvp) { auto k = k_gen_loss<true, true>; PROMP_LAUNCH(k, grid, 256, gen_loss_smem(g.A), st, g, 0); }
    else if (fwd_only) { auto k = k_gen_loss<false, false>; PROMP_LAUNCH(k, grid, 256, gen_loss_smem(g.A), st, g, 0); }
    else { auto k = k_gen_loss<false, true>; PROMP_LAUNCH(k, grid, 256, gen_loss_smem(g.A), st, g, 0); }
    int pp = 0;
    for (int li = c->n_lin - 1; li >= 0 && !fwd_only; --li) {
        const int nbw = (c->lin[li].N + 63) / 64;
        PROMP_GEN_NBW(nbw, if (hvp) gen_wgrad<2, NBW>(c, S, g, li, pp); else gen_wgrad<1, NBW>(c, S, g, li, pp);)
        if (li == 0) break;
        const int nbk = (c->lin[li].K + 63) / 64;
        PROMP_GEN_NBW(nbk, if (hvp) gen_linear<GEN_BWD_T, NBW>(c, lgrid, g, li, pp); else gen_linear<GEN_BWD, NBW>(c, lgrid, g, li, pp);)
        pp ^= 1;
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// The per-task range of a slab's observations (the FP16 split's scale, promp_kernels_pass.h: k_obs_range), enqueued on `st` behind
// whatever wrote the slab there.  The uploads call it on their own stream (its cost is the upload's); the device-side writers only
// mark the table stale and the first policy pass recomputes it.
int enqueue_obs_range(promp_ctx* c, PassSlab& S, hipStream_t st) {
    if (S.n_rows <= 0) return 0;
    HIPCHECK(hipMemsetAsync(S.obs_absmax, 0, sizeof(unsigned) * c->d.n_tasks, st));
    ObsRangeArgs r;
    r.obs = S.obs; r.task_row_offsets = S.task_row_offsets; r.absmax = S.obs_absmax; r.O = c->d.obs_dim;
    const int slices = (c->n_cus * 2 + c->d.n_tasks - 1) / c->d.n_tasks;
    PROMP_LAUNCH(k_obs_range, dim3(slices < 1 ? 1 : slices > 32 ? 32 : slices, c->d.n_tasks), 256, 16, st, r);
    HIPCHECK(hipGetLastError());
    S.obs_range_valid = true;
    c->wbp.valid = false;          // (the hidden_0 planes carry the scales this launch rewrites)
    return 0;
}

// Does the gradient pass fill the primal cache for the R-operator pass behind it?  Only the Chain family keeps one (the cooperative
// kernels keep theta' and the scalars only).  promp_set_primal_cache: 1 / 0; -1 (default) = yes at every size.  Through round 5 the
// default was "from two rounds of tiles per compute unit" (a small shard's passes are all fixed cost and the stores cost what the
// R-operator pass got back: 0.750 vs 0.737 ms per step at 5 tasks).  Since the cache-reading instance runs every product on the
// FP16 pipe (round 6: 12.2 k cycles per tile against 26.3 k for the recomputing one) the cache pays on small shards too: 0.516 vs
// 0.545 ms at 5 tasks, 0.475 vs 0.485 at 3 (two A/B pairs, one box).
static bool primal_cache_on(const promp_ctx* c) { return c->family == PassFamily::Chain && c->primal_cache != 0; }
// the slab's primal cache (promp_kernels_chain.h: chain_cache_row), allocated on first use
static int ensure_primal_cache(promp_ctx* c, PassSlab& S) {
    if (S.hcache) return 0;
    return S.hcache.alloc((S.cache_rows + 16 * (size_t)c->d.n_tasks) * chain_cache_row(c->d.hidden1, c->d.hidden2));
}

// Chain: k_chain_hvp reduces in-launch when a.fuse_reduce says so; k_pass is followed by k_reduce_task
static void launch_chain(promp_ctx* c, PassSlab& S, const PassArgs& a, const PassReq& q, int cache) {
    const int n1 = c->d.hidden1 / 16, n2 = c->d.hidden2 / 16, ks = chain_ksteps(c->d.obs_dim);
    const dim3 grid(S.n_chain_wg);
    if (q.hvp) {
#define PROMP_CHAIN_CASE(N1, N2, KS)                                                                                             \
    if (n1 == N1 && n2 == N2 && ks == KS) {                                                                                      \
        if (cache == 2) { auto k = k_chain_hvp<N1, N2, KS, CHAIN_NW_HVP, true>; PROMP_LAUNCH(k, grid, 64 * CHAIN_NW_HVP, c->smem_hvp, c->stream, a); } \
        else { auto k = k_chain_hvp<N1, N2, KS, CHAIN_NW_HVP, false>; PROMP_LAUNCH(k, grid, 64 * CHAIN_NW_HVP, c->smem_hvp, c->stream, a); }           \
    }
        PROMP_CHAIN_ALL(PROMP_CHAIN_CASE)
#undef PROMP_CHAIN_CASE
        return;
    }
#define PROMP_PASS_CASE(N1, N2)                                                                                                          \
    if (n1 == N1 && n2 == N2) {                                                                                                          \
        if (q.fwd_only) { auto k = k_pass<N1, N2, CHAIN_NW_HVP, false, false>; PROMP_LAUNCH(k, grid, 64 * CHAIN_NW_HVP, c->smem_fwd, c->stream, a); }   \
        else if (cache == 1) { auto k = k_pass<N1, N2, CHAIN_NW_HVP, true, true>; PROMP_LAUNCH(k, grid, 64 * CHAIN_NW_HVP, c->smem_fwd, c->stream, a); } \
        else { auto k = k_pass<N1, N2, CHAIN_NW_HVP, true, false>; PROMP_LAUNCH(k, grid, 64 * CHAIN_NW_HVP, c->smem_fwd, c->stream, a); }            \
    }
    PROMP_PASS_ALL(PROMP_PASS_CASE)
#undef PROMP_PASS_CASE
}

// CoopFp32: hidden 128, or hidden 64 with obs_dim > 32 (promp_kernels_policy_wide.h)
static void launch_coop_fp32(promp_ctx* c, PassSlab& S, const PassArgs& a, const PassReq& q) {
    const int nob = wide_nob(c->d.obs_dim);
    const size_t sm = q.hvp ? c->smem_hvp : c->smem_fwd;
#define PROMP_WIDE_CASE(HH, NOB)                                                                                                \
    if (c->d.hidden1 == HH && nob == NOB) {                                                                                     \
        if (q.hvp) { auto k = k_wide_hvp<HH, NOB>; PROMP_LAUNCH(k, dim3(S.n_work), 4 * HH, sm, c->stream, a); }                 \
        else if (q.fwd_only) { auto k = k_wide_fwd_bwd<HH, NOB, false>; PROMP_LAUNCH(k, dim3(S.n_work), 4 * HH, sm, c->stream, a); } \
        else { auto k = k_wide_fwd_bwd<HH, NOB, true>; PROMP_LAUNCH(k, dim3(S.n_work), 4 * HH, sm, c->stream, a); }             \
    }
    PROMP_WIDE_ALL(PROMP_WIDE_CASE)
#undef PROMP_WIDE_CASE
}

// CoopSplit: two layers of 128 units on the BF16 matrix pipe (promp_kernels_wide_bf16.h), behind the small launches that lay the
// parameters' (and the direction's) hidden kernels out as BF16 planes in fragment order (276 KB per task)
static void launch_coop_split(promp_ctx* c, PassSlab& S, PassArgs& a, const PassReq& q) {
    const int nko = wb_nko(c->wb_cls);
    WbPlaneArgs pa;
    const bool at_meta = q.theta == c->theta && q.theta_stride == 0 && c->wb_planes_meta;
    const bool standing = at_meta && c->wbp.valid && c->wbp.theta_version == c->theta_version && c->wbp.data_version == S.data_version &&
                          c->wbp.sizes_version == c->sizes_version && c->wbp.step == (const void*)&S;
    pa.src = q.theta; pa.src_stride = q.theta_stride; pa.dst = at_meta ? c->wb_planes_meta : c->wb_planes; pa.O = c->d.obs_dim; pa.A = c->d.act_dim; pa.NKO = nko; pa.row_sign = 1.f;
    pa.obs_absmax = a.obs_absmax; pa.vec_absmax = nullptr;       // FP16 split: the hidden_0 kernel takes the inverse of the observations' scale
    // (one copy per task even when the tasks share their parameters: the hidden_0 kernel's planes carry the task's observation scale)
    const bool per_task = q.theta_stride != 0 || PROMP_NT == 2;
    if (!standing) PROMP_LAUNCH(k_wb_planes, dim3((4 * (nko + 16) * 64 + 256 + 255) / 256, per_task ? c->d.n_tasks : 1), 256, 0, c->stream, pa);
    if (at_meta) {
        c->wbp.valid = true; c->wbp.theta_version = c->theta_version; c->wbp.data_version = S.data_version;
        c->wbp.sizes_version = c->sizes_version; c->wbp.step = (const void*)&S;
    }
    a.wb_theta_planes = pa.dst;
    a.wb_plane_stride = per_task ? wb_planes_words(nko) : 0;
    if (q.hvp) {
        // the direction's planes carry its scale: its largest entry per task first (one small launch)
        VecAbsmaxArgs va;
        va.src = c->vbuf; va.stride = c->NP; va.n = c->NP; va.out = c->vdir_absmax;
        va.n_w1 = mlp2_layout(c->d.obs_dim, c->d.hidden1, c->d.hidden2, c->d.act_dim).b1; va.obs_absmax = a.obs_absmax;
        PROMP_LAUNCH(k_vec_absmax, dim3(c->d.n_tasks), 1024, 64, c->stream, va);
        a.vdir_absmax = (const float*)c->vdir_absmax.p;
        pa.src = c->vbuf; pa.src_stride = c->NP; pa.dst = c->wb_vplanes; pa.vec_absmax = a.vdir_absmax;
        PROMP_LAUNCH(k_wb_planes, dim3((4 * (nko + 16) * 64 + 256 + 255) / 256, c->d.n_tasks), 256, 0, c->stream, pa);
        a.wb_v_planes = c->wb_vplanes;
    }
#define PROMP_WB_CASE(CLS, NKO, NXB)                                                                                              \
    if (c->wb_cls == CLS) {                                                                                                       \
        if (q.hvp) { auto k = k_wb_hvp<NKO, NXB>; PROMP_LAUNCH(k, dim3(S.n_work), 256, c->smem_wb_hvp, c->stream, a); }           \
        else if (q.fwd_only) { auto k = k_wb_fwd_bwd<NKO, NXB, false>; PROMP_LAUNCH(k, dim3(S.n_work), 256, c->smem_wb_fwd, c->stream, a); } \
        else { auto k = k_wb_fwd_bwd<NKO, NXB, true>; PROMP_LAUNCH(k, dim3(S.n_work), 256, c->smem_wb_bwd, c->stream, a); }       \
    }
    PROMP_WB_ALL(PROMP_WB_CASE)
#undef PROMP_WB_CASE
}

// One policy pass over a slab plus the per-task reduction that consumes it (q.red_mode, promp_kernels_chain.h).
// k_chain_hvp can do both in one launch; every other pass kernel is followed by k_reduce_task.
int launch_pass(promp_ctx* c, PassSlab& S, const PassReq& q) {
    if (!S.has_policy) return fail(-3, "step has no actions / agent_infos uploaded");
    if (!S.has_adv) return fail(-3, "step has no advantages: call promp_process_samples or promp_set_advantages first");
    if (!S.obs_range_valid && enqueue_obs_range(c, S, c->stream)) return -2;
    const bool chain = c->family == PassFamily::Chain;
    PassArgs a;
    memset(&a, 0, sizeof a);
    a.obs_absmax = (const float*)S.obs_absmax;
    a.obs = S.obs; a.act = S.act; a.adv = q.adv ? q.adv : S.adv; a.old_mean = S.old_mean; a.old_log_std = S.old_ls;
    a.row_tan = q.hvp ? q.row_tan : nullptr;
    const int cache = (!chain || q.fwd_only || !S.hcache) ? 0 : q.cache;
    a.hcache = cache ? S.hcache.p : nullptr;
    if (cache == 1) S.cache_tag = ++c->cache_counter;
    a.ls_per_row = S.ls_per_row;
    a.task_row_offsets = S.task_row_offsets;
    a.work = S.work;
    a.segs = S.chain_segs; a.wg_seg_offsets = S.chain_wg_offsets;
    a.theta = q.theta; a.theta_task_stride = q.theta_stride;
    a.vdir = c->vbuf;
    a.partials = c->partials; a.partial_stride = c->partial_stride;
    a.O = c->d.obs_dim; a.A = c->d.act_dim;
    a.loss_kind = q.loss_kind; a.clip_eps = q.clip_eps; a.clip_log_std = q.clip_ls;
    a.min_log_std = c->min_log_std;   // GaussianMLPPolicy min_std (policies/gaussian_mlp_policy.py:31,35)
    a.kl_weight = q.klw;
    a.task_counters = c->task_counters; a.task_slot_offsets = S.chain_slot_offsets;
    // In-launch reduction (the last-arriving workgroup of a task sums its partial rows) against the grid-wide k_reduce_task
    // behind the launch: with few tasks every task finishes at once and one workgroup per task streaming ~50 partial rows
    // is exposed (66 us vs 46 + 5 us at 5 tasks); with 40 tasks the sums partly hide under other tasks' tiles, but since
    // k_reduce_task keeps eight rows per thread in flight the separate launch wins there too (123 + 5 us vs 137 us with the
    // primal cache, 147 + 5 vs 162 us without).  The in-launch form stays available (promp_set_schedule).
    a.fuse_reduce = (q.hvp && chain && c->d.n_tasks >= c->fuse_min_tasks) ? 1 : 0;
    float* scal = q.scal ? q.scal : c->scal_tmp;
    a.red_mode = q.red_mode; a.step_sizes = c->step_sizes; a.cur = q.cur; a.cur_task_stride = q.cur_stride; a.next = q.next;
    a.lam = c->lam; a.v = c->vbuf; a.scal = scal;
    a.dbg = c->dbg_enabled ? c->dbg.p : nullptr;
    a.split_events = c->split_events;
    const int id = q.hvp ? PROMP_KERNEL_HVP : q.fwd_only ? PROMP_KERNEL_FWD : PROMP_KERNEL_FWD_BWD;
    // (the timed slot covers the pass with the small launches that prepare its operands: k_wb_planes, k_vec_absmax)
    if (prof_begin(c, id, S.n_rows)) return -2;
    switch (c->family) {
    case PassFamily::Chain: launch_chain(c, S, a, q, cache); break;
    case PassFamily::CoopFp32: launch_coop_fp32(c, S, a, q); break;
    case PassFamily::CoopSplit: launch_coop_split(c, S, a, q); break;
    case PassFamily::Layered: if (launch_pass_generic(c, S, a, q.hvp, q.fwd_only)) return -2; break;
    }
    HIPCHECK(hipGetLastError());
    if (prof_end(c, id)) return -2;
    if (a.fuse_reduce) return 0;
    ReduceArgs r;
    r.partials = c->partials; r.partial_stride = c->partial_stride;
    // the register-chained kernels write one row per segment
    r.task_wg_offsets = chain ? S.chain_slot_offsets : S.task_wg_offsets;
    r.NP = c->NP;
    r.step_sizes = c->step_sizes; r.mode = q.red_mode;
    r.cur = q.cur; r.cur_task_stride = q.cur_stride; r.next = q.next;
    r.lam = c->lam; r.v = c->vbuf; r.scal = scal;
    r.next2 = q.red_mode == RED_STEP ? q.next2 : nullptr; r.scal2 = q.red_mode == RED_STEP ? q.scal2 : nullptr;
    float* ginner = q.red_mode == RED_STEP ? q.ginner : nullptr;
    if (ginner) PROMP_LAUNCH(k_reduce_task_keep, dim3((c->NP + 2 + 255) / 256, c->d.n_tasks), 256, 0, c->stream, r, ginner);
    else PROMP_LAUNCH(k_reduce_task, dim3((c->NP + 2 + 255) / 256, c->d.n_tasks), 256, 0, c->stream, r);
    HIPCHECK(hipGetLastError());
    return 0;
}

// (the DiCE objective's gradient is the log-likelihood objective's with the suffix-sum weights of promp_set_dice_rewards)
int loss_kind_inner(int inner_kind) { return (inner_kind == PROMP_INNER_LOGLIK || inner_kind == PROMP_INNER_DICE) ? LOSS_LOGLIK : LOSS_RATIO; }
int loss_kind_outer(int outer_kind) {
    return outer_kind == PROMP_OUTER_RATIO ? LOSS_RATIO : outer_kind == PROMP_OUTER_KL ? LOSS_KL
           : outer_kind == PROMP_OUTER_LOGLIK ? LOSS_LOGLIK : LOSS_CLIP;
}

// promp_inner_adapt has left the first inner pass's results behind (theta' in chain[1], its scalars, the primal cache) and nothing
// it read has changed since; the clip of log_std at log(min_std) -- the one difference between the two -- is not active
static bool adapt0_stands(const promp_ctx* c, int inner_kind, bool cached) {
    return c->reuse_adapt && c->adapt0.valid && c->adapt0.theta_version == c->theta_version &&
           c->adapt0.data_version == c->steps[0].data_version && c->adapt0.sizes_version == c->sizes_version &&
           c->adapt0.inner_kind == inner_kind && c->adapt0.cached == cached && c->adapt0.min_log_std == c->min_log_std &&
           c->adapt0.learn_std == c->learn_std && c->ls_known && c->ls_min >= c->min_log_std;
}

// The one exchange of the path (meta_algos/pro_mp.py:122,151,155: the mean over tasks): the ranks' sums of n floats, in place.
//   default      ncclAllReduce -- the result is the same on every rank for a given algorithm / topology, but the ORDER of the
//                additions is RCCL's;
//   fixed_order  ncclAllGather of the ranks' vectors + k_sum_ranks adding them in rank order 0, 1, ... on every rank: replicas
//                bitwise identical by construction, and equal to what one process adding its shards in that order computes
//                (the fixed-order one-shot variant; n is ~6 k floats, the gather moves nranks x 24 KB).
static int exchange_sums_raw(promp_ctx* c, float* buf, size_t n);
static int exchange_sums(promp_ctx* c, float* buf, size_t n) {
    if (!c->comm) return 0;
    // (promp_prof_enable: HIP events around the exchange on the stream it is enqueued on -- the per-call latency bench.py reports)
    if (prof_begin(c, PROMP_KERNEL_EXCHANGE, 0)) return -2;
    const int rc = exchange_sums_raw(c, buf, n);
    if (rc) return rc;
    return prof_end(c, PROMP_KERNEL_EXCHANGE);
}
static int exchange_sums_raw(promp_ctx* c, float* buf, size_t n) {
    if (c->fixed_order) {
        if (c->gather.reserve((size_t)c->nranks * n, 1)) return -2;
        ncclResult_t r = ncclAllGather(buf, c->gather, n, ncclFloat, c->comm, c->stream);
        if (r != ncclSuccess) return fail(-4, "ncclAllGather failed: %s", ncclGetErrorString(r));
        PROMP_LAUNCH(k_sum_ranks, dim3((unsigned)((n + 255) / 256)), 256, 0, c->stream, (const float*)c->gather, buf, (int)n, c->nranks);
        HIPCHECK(hipGetLastError());
        return 0;
    }
    ncclResult_t r = ncclAllReduce(buf, buf, n, ncclFloat, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) return fail(-4, "ncclAllReduce failed: %s", ncclGetErrorString(r));
    return 0;
}

// A context that holds a shard of the meta-batch (n_tasks_global > n_tasks) but no communicator: the external-collective mode.
// Its entry points return this rank's SHARE of a mean (promp_meta_grad: local sums / n_tasks_global, the sums themselves in the
// exchange buffer); the ones that would go on to USE a mean (an Adam step, a conjugate-gradient product) refuse instead.
static bool sharded_without_comm(const promp_ctx* c) { return c->d.n_tasks_global > c->d.n_tasks && c->comm == nullptr; }

// what the *_ss instances of the final stage take beside theta's arguments (promp_kernels_step_sizes.h)
static StepSizeArgs step_size_args(const promp_ctx* c) {
    StepSizeArgs s;
    s.galpha = c->galpha; s.alpha = c->step_sizes; s.alpha_m = c->ss_m; s.alpha_v = c->ss_v; s.alpha_grad_mean = c->ss_grad;
    return s;
}

// ---- the final stage of an evaluation (promp_kernels_policy.h), launched from final_stage_launch's decision (promp_plan.h) ----
static FinalLaunch final_launch(const promp_ctx* c, bool stepping, bool split_wanted, bool sizes) {
    return final_stage_launch(final_stage_plan(c->outer, c->sw, stepping, split_wanted), c->NP, c->d.num_inner_steps, sizes);
}
// The mean kernels' arguments: everything but lr_t (outer_step_begins).  stats: the slot to write; publish: promp_optimize_begin's
// last launch.
static AdamArgs adam_args(const promp_ctx* c, float* stats, const float* eta, bool publish, bool do_update) {
    AdamArgs ad;
    ad.theta = c->theta; ad.m = c->adam_m; ad.v = c->adam_v; ad.red = c->red; ad.grad_mean = c->grad_mean;
    ad.stats = stats; ad.NP = c->NP; ad.K = c->d.num_inner_steps; ad.A = c->d.act_dim;
    for (int k = 0; k < PROMP_ETA_MAX; ++k) ad.eta[k] = k < ad.K ? eta[k] : 0.f;
    ad.host_stats = publish ? c->stats_host.p : nullptr; ad.host_seq = c->stats_seq_host; ad.seq = c->stats_seq;
    ad.inv_tasks = 1.0f / (float)c->d.n_tasks_global;
    ad.do_update = do_update ? 1 : 0;
    ad.n_trainable = c->learn_std ? c->NP : c->NP - c->d.act_dim;
    ad.lr_t = 0.f;
    return ad;
}
// A step is about to be enqueued: what was derived from theta (and, sizes, from the step sizes) is stale, the smallest log_std
// entry is unknown until the next publication, and the step count advances.  Returns the lr_t the launch carries.
static float outer_step_begins(promp_ctx* c, bool sizes, float lr) {
    c->theta_version = ++c->version_counter;
    if (sizes) c->sizes_version = ++c->version_counter;
    c->ls_known = false;
    c->adam_t += 1;
    return outer_lr_t(c->outer, lr, c->adam_t);
}
// One launch of the final stage.  f alone: the task sums (the split route's first half; promp_constraint_hvp); ad alone: mean +
// step on the exchanged sums (its second half; promp_adam_step); both: sum + step in one launch.
static int launch_final_stage(promp_ctx* c, const FinalLaunch& L, const FinalArgs* f, const AdamArgs* ad) {
    const StepSizeArgs ss = step_size_args(c);
    const OuterOptArgs oo = outer_opt_args(c->outer);
    hipStream_t s = c->stream;
    if (!ad) {
        if (L.sizes) PROMP_LAUNCH(k_reduce_final_ss, dim3(L.reduce_grid), 256, 0, s, *f, ss.galpha);
        else PROMP_LAUNCH(k_reduce_final, dim3(L.reduce_grid), 256, 0, s, *f);
    } else if (!f) {
        if (L.general && L.sizes) PROMP_LAUNCH(k_mean_outer_ss, dim3(L.mean_grid), 256, 0, s, *ad, ss, oo, c->grad_norm.p);
        else if (L.general) PROMP_LAUNCH(k_mean_outer, dim3(L.mean_grid), 256, 0, s, *ad, oo, c->grad_norm.p);
        else if (L.sizes) PROMP_LAUNCH(k_mean_adam_ss, dim3(L.mean_grid), 256, 0, s, *ad, ss);
        else PROMP_LAUNCH(k_mean_adam, dim3(L.mean_grid), 256, 0, s, *ad);
    } else {
        if (L.general && L.sizes) PROMP_LAUNCH(k_final_outer_ss, dim3(L.fused_grid), 256, 0, s, *f, *ad, ss, oo);
        else if (L.general) PROMP_LAUNCH(k_final_outer, dim3(L.fused_grid), 256, 0, s, *f, *ad, oo);
        else if (L.sizes) PROMP_LAUNCH(k_final_adam_ss, dim3(L.fused_grid), 256, 0, s, *f, *ad, ss);
        else PROMP_LAUNCH(k_final_adam, dim3(L.fused_grid), 256, 0, s, *f, *ad);
    }
    if (ad && L.general && oo.max_norm > 0.f) c->norm_valid = true;
    HIPCHECK(hipGetLastError());
    return 0;
}

// The step as a policy pass is to see it.  The counts, flags and version that the step's entry points keep in StepData reach
// the slab HERE and nowhere else; what the passes themselves write (obs_range_valid, the primal cache) lives in the slab alone.
static PassSlab& pass_slab(StepData& S) {
    PassSlab& ps = S.ps;
    ps.n_rows = S.n_rows; ps.n_work = S.n_work[0]; ps.n_chain_wg = S.n_chain_wg;
    ps.ls_per_row = S.ls_per_row; ps.has_policy = S.has_policy; ps.has_adv = S.has_adv; ps.data_version = S.data_version;
    return ps;
}
static EvalSet full_set(promp_ctx* c) {
    EvalSet E{{}, c->steps.data(), c->chain, c->scal_inner, &c->chvp};
    for (size_t k = 0; k < c->steps.size(); ++k) E.slab[k] = &pass_slab(c->steps[k]);
    return E;
}

// One evaluation of the meta-objective (+ gradient, + Adam) enqueued on the stream.  sizes_grad: with trainable step sizes the
// gradient evaluation also leaves the step sizes' gradient (and Adam steps them); promp_cg_solve's evaluations say no.
int enqueue_meta_on(promp_ctx* c, const EvalSet& E, float clip_eps, const float* eta_host, int inner_kind, int outer_kind,
                    bool want_grad, bool do_adam, float lr, bool sizes_grad) {
    PassSlab* const* W = E.slab;
    const int K = c->d.num_inner_steps, M = c->d.n_tasks, NP = c->NP;
    const size_t MNP = (size_t)M * NP;
    const bool ag = c->train_sizes && want_grad && sizes_grad;
    for (int k = 0; k <= K; ++k)
        if (W[k]->n_rows == 0) return fail(-3, "step %d has no data", k);
    // a step's second-stream sample processing is waited for right in front of the first pass that reads its advantages:
    // the passes on earlier steps run while it finishes
    if (!E.full && ag) c->adapt0.valid = false;      // (ginner[0] is about to hold the selection's gradient)
    bool filled[PROMP_ETA_MAX] = {};      // steps whose primal cache this evaluation has written
    for (int k = 0; k < K; ++k) {
        const float* th = (k == 0) ? c->theta : E.chain + (size_t)k * MNP;
        const long long st = (k == 0) ? 0 : NP;
        if (E.full && join_side(c, E.full[k])) return -2;
        // the R-operator pass of this step (below) runs at these parameters on this slab: it reads the activations and means
        // back instead of recomputing them (primal cache, promp_kernels_chain.h)
        const bool cached = want_grad && primal_cache_on(c);
        if (cached && ensure_primal_cache(c, *W[k])) return -2;
        // promp_inner_adapt has left exactly this pass's results behind (see there) if nothing it read has changed since and
        // the clip of log_std at log(min_std) -- the one difference between the two -- is not active
        const bool reuse = k == 0 && E.full && adapt0_stands(c, inner_kind, cached);
        if (reuse) {                               // (with trainable step sizes it left its gradient in ginner[0] as well)
            c->adapt_passes_skipped += 1;
            filled[k] = cached;
            continue;
        }
        PassReq q;
        q.theta = th; q.theta_stride = st; q.loss_kind = loss_kind_inner(inner_kind); q.clip_eps = clip_eps; q.clip_ls = k == 0;
        q.red_mode = RED_STEP; q.cur = th; q.cur_stride = st; q.next = E.chain + (size_t)(k + 1) * MNP; q.scal = E.scal_inner + (size_t)k * M * 2;
        q.cache = cached ? 1 : 0;
        q.ginner = ag ? c->ginner + (size_t)k * MNP : nullptr;
        if (launch_pass(c, *W[k], q)) return -2;
        filled[k] = cached;
    }
    if (E.full && join_side(c, E.full[K])) return -2;
    {
        PassReq q;
        q.theta = E.chain + (size_t)K * MNP; q.theta_stride = NP; q.loss_kind = loss_kind_outer(outer_kind); q.clip_eps = clip_eps;
        q.fwd_only = !want_grad; q.red_mode = want_grad ? RED_OUTER : RED_SCAL; q.scal = c->scal_outer;
        if (launch_pass(c, *W[K], q)) return -2;
    }
    if (want_grad) {
        for (int k = K - 1; k >= 0; --k) {
            const float* th = (k == 0) ? c->theta : E.chain + (size_t)k * MNP;
            const long long st = (k == 0) ? 0 : NP;
            PassSlab& Sk = *W[k];
            const bool dice = inner_kind == PROMP_INNER_DICE;     // (the step's coupling rows: compact sets are refused before)
            if (dice && !(E.full && E.full[k].has_dice)) return fail(-3, "step %d has no DiCE rewards: call promp_set_dice_rewards first", k);
            if (ag) {
                // lam is the complete multiplier of theta_{k+1} here, both pieces of a DiCE step included
                PROMP_LAUNCH(k_step_size_grad, dim3((NP + 255) / 256, M), 256, 0, c->stream, c->galpha.p, (const float*)c->lam,
                             (const float*)(c->ginner + (size_t)k * MNP), NP, k == K - 1 ? 1 : 0);
                HIPCHECK(hipGetLastError());
            }
            PassReq q;
            q.hvp = true; q.theta = th; q.theta_stride = st; q.loss_kind = loss_kind_inner(inner_kind); q.clip_eps = clip_eps; q.clip_ls = k == 0;
            q.klw = dice ? 0.f : eta_host[k] / (float)K; q.red_mode = RED_HVP;
            q.cache = filled[k] ? 2 : 0; q.row_tan = dice ? E.full[k].dice_c.p : nullptr;
            if (launch_pass(c, Sk, q)) return -2;
            if (dice) {
                // The magic box couples the time steps of a path: H v = H_loglik(w) v + grad_loglik(u(v)), u from the row tangents
                // c_t = dlogpi_t . v of the pass above (meta_algos/dice_maml.py:245-258).  The pass ran on the direction -v, so its
                // tangents and with them u carry the sign that makes the second piece ANOTHER "lam += g" reduction.
                const StepData& D = E.full[k];
                DiceScanArgs ds;
                ds.path_row_offsets = D.path_row_offsets; ds.rw = D.dice_rw; ds.c = D.dice_c; ds.out = D.dice_u; ds.tmp = D.dice_tmp;
                ds.mode = 1;
                PROMP_LAUNCH(k_dice_scan, dim3(D.n_paths), 64, 0, c->stream, ds);
                HIPCHECK(hipGetLastError());
                PassReq qc;
                qc.theta = th; qc.theta_stride = st; qc.loss_kind = LOSS_LOGLIK; qc.clip_ls = k == 0; qc.red_mode = RED_HVP; qc.adv = D.dice_u;
                if (launch_pass(c, Sk, qc)) return -2;
            }
        }
    }
    FinalArgs f;
    f.lam = c->lam; f.NP = NP; f.K = K; f.n_tasks = M;
    f.scal_inner = E.scal_inner; f.scal_outer = c->scal_outer; f.red = c->red; f.want_grad = want_grad ? 1 : 0;
    c->red_has_sizes = ag;
    // several ranks (or an external collective: more global than local tasks): sums first, mean + step after the exchange;
    // a clipped step as well (the norm of ALL entries comes first), and settings that are not the default ones step in the
    // general kernels (final_stage_plan).  One rank: nothing in between, one launch.
    const FinalLaunch L = final_launch(c, do_adam, c->nranks > 1 || c->force_split || c->d.n_tasks_global != c->d.n_tasks, ag);
    if (L.split) {
        if (launch_final_stage(c, L, &f, nullptr)) return -2;
        if (exchange_sums(c, c->red, L.red_count)) return -4;      // (one exchange per epoch, with or without the step sizes)
    }
    AdamArgs ad = adam_args(c, c->stats + (size_t)c->stats_slot * (K + 2), eta_host, c->publish_next, do_adam);
    if (do_adam) ad.lr_t = outer_step_begins(c, ag, lr);
    if (launch_final_stage(c, L, L.split ? nullptr : &f, &ad)) return -2;
    for (int k = 0; k <= K && E.full; ++k) E.full[k].dirty = true;
    return 0;
}
int enqueue_meta(promp_ctx* c, float clip_eps, const float* eta_host, int inner_kind, int outer_kind, bool want_grad,
                 bool do_adam, float lr, bool sizes_grad = true) {
    return enqueue_meta_on(c, full_set(c), clip_eps, eta_host, inner_kind, outer_kind, want_grad, do_adam, lr, sizes_grad);
}

int upload_eta(promp_ctx* c, const float* eta) {
    // the coefficients travel by value in the launch arguments of the final reduction; promp_adam_step reuses the last set
    for (int k = 0; k < c->d.num_inner_steps; ++k) c->eta_last[k] = eta[k];
    return 0;
}

int alloc_step(promp_ctx* c, StepData& S) {
    const promp_dims* dims = &c->d;
    const int M = dims->n_tasks;
    const size_t R = dims->max_rows, P = dims->max_paths, A = dims->act_dim, O = dims->obs_dim;
    if (S.obs.alloc(R * O) || S.act.alloc(R * A) || S.rew.alloc(R)) return -2;
    if (S.obs_absmax.alloc((size_t)M)) return -2;
    if (S.old_mean.alloc(R * A) || S.old_ls.alloc(R * A)) return -2;
    if (S.ret32.alloc(R) || S.adv32.alloc(R) || S.ret64.alloc(R) || S.adv64.alloc(R)) return -2;
    if (S.path_row_offsets.alloc(P + 1) || S.path_task.alloc(P) || S.row_t.alloc(R)) return -2;
    if (S.task_row_offsets.alloc((size_t)M + 1) || S.task_path_offsets.alloc((size_t)M + 1)) return -2;
    if (S.task_wg_offsets[0].alloc((size_t)M + 1) || S.task_wg_offsets[1].alloc((size_t)M + 1)) return -2;
    if (S.chain_segs.alloc((size_t)c->max_work) || S.chain_wg_offsets.alloc((size_t)c->max_work + 1)) return -2;
    if (S.chain_slot_offsets.alloc((size_t)M + 1)) return -2;
    if (S.path_ret0.alloc(P) || S.path_undisc.alloc(P) || S.path_rsq.alloc(P)) return -2;
    if (S.path_mom.alloc(3 * P) || S.coeffs.alloc((size_t)M * c->coeff_stride)) return -2;
    if (S.work[0].alloc((size_t)c->max_work) || S.work[1].alloc((size_t)c->max_work)) return -2;
    for (Event* ev : {&S.ev_use, &S.ev_done, &S.ev_ready}) HIPCHECK(hipEventCreateWithFlags(&ev->h, hipEventDisableTiming));
    // what a policy pass reads of the step (the buffers stay where they are for the step's life, and travel with it in a swap)
    PassSlab& ps = S.ps;
    ps.obs = S.obs; ps.act = S.act; ps.adv = S.adv32; ps.old_mean = S.old_mean; ps.old_ls = S.old_ls; ps.obs_absmax = S.obs_absmax;
    ps.task_row_offsets = S.task_row_offsets; ps.task_wg_offsets = S.task_wg_offsets[0]; ps.chain_slot_offsets = S.chain_slot_offsets;
    ps.chain_wg_offsets = S.chain_wg_offsets; ps.work = S.work[0]; ps.chain_segs = S.chain_segs;
    ps.cache_rows = R;
    return 0;
}

// ---- compact slabs: copies of some of a step's paths, laid out as an upload of those paths alone would be -------------------
// Two producers -- a step's selection (one slab; the other paths go nowhere) and its partition into minibatches (B slabs) -- and
// one mechanism: a SlabPool, a table block (promp_plan.h: TableBlock) that one copy sends, one k_scatter_partition launch.
// Room in `pool` for `rows` rows of every array (log_std among them if the step keeps one row per row), the block and B range rows.
int pool_reserve(promp_ctx* c, SlabPool& pool, size_t rows, bool ls_rows, const TableBlock& blk, int B) {
    const size_t O = c->d.obs_dim, A = c->d.act_dim, n_absmax = (size_t)B * c->d.n_tasks;
    if (rows > pool.cap_rows || (ls_rows && !pool.ls_rows)) {
        if (pool.obs.alloc(rows * O) || pool.act.alloc(rows * A) || pool.adv.alloc(rows) || pool.mean.alloc(rows * A)) return -2;
        if (ls_rows && pool.ls.alloc(rows * A)) return -2;
        if (!ls_rows) HIPCHECK(pool.ls.release());
        pool.cap_rows = rows; pool.ls_rows = ls_rows;
    }
    if (blk.total > pool.cap_tables) {
        if (pool.tables.alloc(blk.total)) return -2;
        pool.cap_tables = blk.total;
    }
    if (n_absmax > pool.cap_absmax) {
        if (pool.absmax.alloc(n_absmax)) return -2;
        pool.cap_absmax = n_absmax;
    }
    return 0;
}
// a primal cache sized for fewer rows than the slab is about to hold goes; the next storing pass allocates one that fits
int grow_cache_rows(PassSlab& S, size_t rows) {
    if (rows <= S.cache_rows) return 0;
    HIPCHECK(S.hcache.release());
    S.cache_rows = rows;
    return 0;
}
// a slab's pass tables and counts: its part `s` of a table block on the device, packed from t (pack_slab_tables)
void bind_tables(PassSlab& S, const int* s, const TableBlock& blk, const StepTables& t) {
    S.task_row_offsets = s + blk.tro; S.task_wg_offsets = s + blk.two; S.chain_slot_offsets = s + blk.slot;
    S.chain_wg_offsets = s + blk.wg_off;
    S.work = reinterpret_cast<const WorkItem*>(s + blk.work); S.chain_segs = reinterpret_cast<const ChainSeg*>(s + blk.segs);
    S.n_rows = (int)t.row_t.size(); S.n_work = (int)t.work[0].size(); S.n_chain_wg = (int)t.wg_off.size() - 1;
}
// Behind the copy of step P's table block into pool.tables: the copy launch, and the B slabs as the passes enqueued next are to
// see them -- slab j at row at[j] of the pool, with the tables of tables[j], the step's flags and version, its ranges in place.
// timed: the launch counts in PROMP_KERNEL_SCATTER's profiling slot.
int scatter_slabs(promp_ctx* c, StepData& P, SlabPool& pool, const TableBlock& blk, int B, const size_t* at, const StepTables* tables,
                  PassSlab* slabs, bool timed) {
    const int M = c->d.n_tasks;
    const size_t O = c->d.obs_dim, A = c->d.act_dim;
    hipStream_t st = c->stream;
    HIPCHECK(hipMemsetAsync(pool.absmax, 0, sizeof(unsigned) * B * M, st));
    ScatterPartitionArgs g;
    g.obs_in = P.obs; g.act_in = P.act; g.adv_in = P.adv32; g.mean_in = P.old_mean; g.ls_in = P.ls_per_row ? P.old_ls.p : nullptr;
    g.obs = pool.obs; g.act = pool.act; g.adv = pool.adv; g.mean = pool.mean; g.ls = pool.ls;
    g.src_row_offsets = P.path_row_offsets; g.path_task = P.path_task;
    g.copy = pool.tables; g.shift = pool.tables + blk.shift; g.absmax = pool.absmax;
    g.O = (int)O; g.A = (int)A; g.n_tasks = M;
    if (timed && prof_begin(c, PROMP_KERNEL_SCATTER, P.n_rows)) return -2;
    PROMP_LAUNCH(k_scatter_partition, dim3(P.n_paths), 256, 0, st, g);
    HIPCHECK(hipGetLastError());
    if (timed && prof_end(c, PROMP_KERNEL_SCATTER)) return -2;
    P.dirty = true;
    c->wbp.valid = false;              // (the hidden_0 planes carry the observation scales this launch rewrites)
    for (int j = 0; j < B; ++j) {
        PassSlab& S = slabs[j];
        S.obs = pool.obs + at[j] * O; S.act = pool.act + at[j] * A; S.adv = pool.adv + at[j]; S.old_mean = pool.mean + at[j] * A;
        // (log_std of one row per task: every slab reads the step's own table)
        S.old_ls = P.ls_per_row ? pool.ls + at[j] * A : P.old_ls.p;
        S.obs_absmax = pool.absmax + (size_t)j * M;
        bind_tables(S, pool.tables + blk.slab(j), blk, tables[j]);
        S.ls_per_row = P.ls_per_row; S.has_policy = P.has_policy; S.has_adv = P.has_adv;
        S.data_version = P.data_version;
        S.obs_range_valid = true;      // (k_scatter_partition has left the slab's ranges)
    }
    return 0;
}

// ---- selections: subsampled constraint products -----------------------------------------------------------------------
// Whatever replaces a step's layout drops its selection: old indices never address new rows.
void clear_selection(promp_ctx* c, int step) {
    if ((size_t)step >= c->sel.size() || !c->sel[step].on) return;
    c->sel[step].on = false;
    c->sel[step].gathered = false;
    c->chvp_sel.valid = false;
}
int n_selected(const promp_ctx* c) {
    int n = 0;
    for (const Selection& L : c->sel) n += L.on ? 1 : 0;
    return n;
}
// The compact slab of step k's selection, current: a pool sized by the selection, its table block on the device, and copies of
// the selected paths' rows taken at the step's present data_version (promp_process_samples / promp_set_advantages after the
// selection are seen).  On the main stream, behind the step's pending side-stream / copy-stream work.
int ensure_sub(promp_ctx* c, int k) {
    StepData& P = c->steps[k];
    Selection& L = c->sel[k];
    if (join_side(c, P)) return -2;
    if (L.gathered && L.gathered_version == P.data_version) return 0;
    const TableBlock blk(P.n_paths, 1, c->d.n_tasks, c->max_work);
    const size_t R = L.tables.row_t.size(), at = 0;
    if (pool_reserve(c, L.pool, R, P.ls_per_row != 0, blk, 1) || grow_cache_rows(c->sub[k], R)) return -2;
    HIPCHECK(hipMemcpyAsync(L.pool.tables, L.image.data(), sizeof(int) * blk.total, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));     // (the image may be replaced by the next selection)
    if (scatter_slabs(c, P, L.pool, blk, 1, &at, &L.tables, &c->sub[k], /*timed=*/false)) return -2;
    L.gathered = true; L.gathered_version = P.data_version;
    return 0;
}
// The evaluation set of the selections, every compact slab current.  Refuses unless every step has a selection (a product over
// some steps' subsamples and other steps' whole slabs is no function anybody asked for) and for the DiCE inner objective
// (TRPO-MAML has none; its coupling rows are not among the copies).
int selection_set(promp_ctx* c, int inner_kind, EvalSet* E) {
    const int K = c->d.num_inner_steps, n = n_selected(c);
    if (n != K + 1) return fail(-3, "%d of %d steps have a selection: set one on every step (promp_set_step_selection) or on none", n, K + 1);
    if (inner_kind == PROMP_INNER_DICE) return fail(-3, "the DiCE inner objective is not evaluated on a selection (TRPO-MAML has no DiCE inner type)");
    for (int k = 0; k <= K; ++k)
        if (c->steps[k].n_rows == 0) return fail(-3, "step %d has no data", k);
    for (int k = 0; k <= K; ++k)
        if (ensure_sub(c, k)) return -2;
    *E = EvalSet{{}, nullptr, c->sel_chain, c->sel_scal_inner, &c->chvp_sel};
    for (int k = 0; k <= K; ++k) E->slab[k] = &c->sub[k];
    return 0;
}

// promp_optimize_begin / promp_optimize_minibatch_begin on a context that holds a shard and no communicator
int refuse_sharded_optimize(const promp_ctx* c) {
    return fail(-3, "this context holds %d of %d tasks and has no communicator: promp_optimize would apply this rank's sums as if they "
                    "were the meta-batch's.  Attach one (promp_comm_init), or run the exchange yourself: promp_meta_grad -> "
                    "promp_reduced_get -> all-reduce -> promp_reduced_set -> promp_adam_step", c->d.n_tasks, c->d.n_tasks_global);
}

// ---- minibatched Adam epochs ------------------------------------------------------------------------------------------------
// the first row of every slab in the pool: multiples of 64 rows (a slab's arrays start aligned like an upload's), at least 16
// rows between two slabs
std::vector<size_t> mb_places(const PartitionLayout& part) {
    const int B = (int)part.lay.size();
    std::vector<size_t> at(B + 1, 0);
    for (int j = 0; j < B; ++j) at[j + 1] = (at[j] + (size_t)(part.row_base[j + 1] - part.row_base[j]) + 16 + 63) & ~(size_t)63;
    return at;
}
// Everything promp_optimize_minibatch_begin allocates, before its first enqueue: the pools and table blocks of every step sized
// for the largest epoch, the (K + 1) x B slabs, the primal caches of the slabs the gradient passes store into, the evaluation
// set's own chain and scalars, the page-locked staging of all table copies.
int mb_reserve(promp_ctx* c, int E, int B, const std::vector<PartitionLayout>& parts, size_t* stage_ints) {
    const int K = c->d.num_inner_steps, M = c->d.n_tasks;
    const size_t MNP = (size_t)M * c->NP;
    if (c->mb_pool.empty()) {
        if (c->mb_chain.alloc((size_t)(K + 1) * MNP) || c->mb_scal_inner.alloc((size_t)K * M * 2)) return -2;
        c->mb_pool.resize(K + 1);
        c->mb.resize(K + 1);
    }
    *stage_ints = 0;
    for (int k = 0; k <= K; ++k) {
        const StepData& P = c->steps[k];
        const TableBlock blk(P.n_paths, B, M, c->max_work);
        if (pool_reserve(c, c->mb_pool[k], (size_t)P.n_rows + 80 * (size_t)B, P.ls_per_row != 0, blk, B)) return -2;
        *stage_ints += (size_t)E * blk.total;
        if ((int)c->mb[k].size() < B) c->mb[k].resize(B);
        for (int j = 0; j < B; ++j) {
            PassSlab& S = c->mb[k][j];
            size_t most = 0;
            for (int e = 0; e < E; ++e) most = std::max(most, parts[(size_t)e * (K + 1) + k].tables[j].row_t.size());
            if (grow_cache_rows(S, most)) return -2;
            if (k < K && primal_cache_on(c) && ensure_primal_cache(c, S)) return -2;
        }
    }
    if (c->mb_stage.reserve(*stage_ints, 1)) return -2;
    return 0;
}
// One (epoch, step): the table block's image in `stage` (page-locked, untouched until the optimisation is collected), its copy,
// the copy launch and the B slabs bound to what it fills.
int mb_enqueue_step(promp_ctx* c, int k, int B, const PartitionLayout& part, int* stage) {
    StepData& P = c->steps[k];
    SlabPool& pool = c->mb_pool[k];
    const TableBlock blk(P.n_paths, B, c->d.n_tasks, c->max_work);
    const std::vector<size_t> at = mb_places(part);
    std::vector<int> shifts(B);
    for (int j = 0; j < B; ++j) shifts[j] = (int)at[j] - part.row_base[j];
    pack_table_block(blk, part.copy, shifts, part.tables.data(), stage);
    if (join_side(c, P)) return -2;
    HIPCHECK(hipMemcpyAsync(pool.tables, stage, sizeof(int) * blk.total, hipMemcpyHostToDevice, c->stream));
    return scatter_slabs(c, P, pool, blk, B, at.data(), part.tables.data(), c->mb[k].data(), /*timed=*/true);
}

}  // namespace

extern "C" {

const char* promp_last_error(void) { return g_err.c_str(); }
int promp_abi_version(void) { return 3; }

int promp_param_count(const promp_dims* d) {
    if (!d) return fail(-1, "dims is NULL");
    return param_count(d);
}
int promp_feature_dim(const promp_dims* d, int kind) {
    if (!d) return fail(-1, "dims is NULL");
    return feature_dim(d, kind);
}

int promp_ctx_create(promp_ctx** out, int device_id, const promp_dims* user_dims) {
    if (!out) return fail(-1, "out is NULL");
    *out = nullptr;
    std::string why;
    if (const int rc = check_dims(user_dims, &why)) return fail_plan(rc, why);
    promp_dims padded_dims;
    pad_dims(user_dims, &padded_dims);
    const promp_dims* dims = &padded_dims;        // everything below sees the instantiated shape
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(-2, "no HIP device available (%s): libpromp_hip has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "0 devices");
    if (device_id < 0 || device_id >= ndev) return fail(-1, "device_id %d out of range (%d devices)", device_id, ndev);
    HIPCHECK(hipSetDevice(device_id));
    // every exit below but the last releases the context and what it holds by then
    std::unique_ptr<promp_ctx, void (*)(promp_ctx*)> guard(new promp_ctx(), promp_ctx_destroy);
    promp_ctx* c = guard.get();
    c->device = device_id;
    c->d = *dims;
    c->du = *user_dims;
    c->NPu = param_count(user_dims);
    c->padded = c->NPu != param_count(dims);
    c->sw = plan_switches_from_env();
    c->gen_bf16 = !c->sw.gen_fp32;
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device_id));
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (c->sw.max_cus > 0 && c->sw.max_cus < c->n_cus) c->n_cus = c->sw.max_cus;
    c->clock_mhz = prop.clockRate / 1000;
    snprintf(c->dev_name, sizeof c->dev_name, "%s", prop.name[0] ? prop.name : PROMP_ARCH_NAME(prop));
    HIPCHECK(hipStreamCreate(&c->stream.h));
    {   // sample processing of steps >= 1 is a string of small latency-bound kernels under a chip-filling pass: with the
        // higher priority their workgroups are placed first, the string finishes before the main stream needs its result
        int lo = 0, hi = 0;
        HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // (PROMP_SIDE_PRIO=lo / none: the A/B switch)
        const char* e = getenv("PROMP_SIDE_PRIO");
        if (e && e[0] == 'n') HIPCHECK(hipStreamCreate(&c->side.h));
        else HIPCHECK(hipStreamCreateWithPriority(&c->side.h, hipStreamDefault, (e && e[0] == 'l') ? lo : hi));
    }
    const int K = dims->num_inner_steps, M = dims->n_tasks;
    c->NP = param_count(dims);
    // (observations wider than PROMP_LINFEAT_MAX_O: the partial Gram blocks of 2 obs_dim + 5 columns outgrow what a context should
    //  hold -- 3.8 MB per work item at obs_dim 480; such contexts fit LinearTimeBaseline / no baseline on the device, or take
    //  advantages through promp_set_advantages)
    c->Dmax = dims->obs_dim <= PROMP_LINFEAT_MAX_O ? 2 * dims->obs_dim + 4 : 4;
    c->coeff_stride = c->Dmax;
    c->max_work = 2 * c->n_cus + M;
    c->partial_stride = (c->NP + PROMP_PARTIAL_EXTRA + 3) & ~3;
    const int nblk_max = (c->Dmax + 1 + 15) / 16;
    c->gram_stride = nblk_max * (nblk_max + 1) / 2 * 256;
    // the pass family, chosen once (pass_family); what follows sizes its launches
    const FamilyPlan fam = pass_family(dims, c->sw);
    c->family = fam.family;
    c->wb_cls = fam.wb_cls;
    switch (c->family) {
    case PassFamily::Layered: {
        const HiddenList L = hidden_list(dims);
        int in = dims->obs_dim, off = 0;
        c->n_lin = L.n + 1;
        c->g_maxw = dims->act_dim;
        for (int l = 0; l <= L.n; ++l) {
            const int out = l < L.n ? L.h[l] : dims->act_dim;
            c->lin[l] = GenLin{in, out, off, off + in * out};
            off += in * out + out;
            if (out > c->g_maxw) c->g_maxw = out;
            in = out;
        }
        for (int l = 0; l < c->n_lin; ++l) {
            c->gb_pf_off[l] = (int)c->gb_plane_stride; c->gb_plane_stride += gb_f_elems(c->lin[l].K, c->lin[l].N);
            c->gb_pb_off[l] = (int)c->gb_plane_stride; c->gb_plane_stride += gb_b_elems(c->lin[l].K, c->lin[l].N);
        }
        break;
    }
    case PassFamily::CoopFp32:
    case PassFamily::CoopSplit: {
        const int nob = wide_nob(dims->obs_dim);
        c->smem_fwd = sizeof(float) * (size_t)make_layout_wide(dims->hidden1, 4, nob, false).total;
        c->smem_hvp = sizeof(float) * (size_t)make_layout_wide(dims->hidden1, 2, nob, true).total;
        // two layers of 128 units: the first-order pass on the BF16 matrix pipe (float32-equivalent 3-way split)
        if (c->family == PassFamily::CoopSplit) {
            c->smem_wb_bwd = sizeof(float) * (size_t)wb_layout(false).total;
            c->smem_wb_fwd = c->smem_wb_bwd;
            c->smem_wb_hvp = sizeof(float) * (size_t)wb_layout(true).total;
        }
        break;
    }
    case PassFamily::Chain:
        c->smem_fwd = sizeof(float) * (size_t)pass_layout(dims->hidden1 / 16, dims->hidden2 / 16, CHAIN_NW_HVP, c->NP).total;
        // (one size for both instances: the cache-reading one lays LDS out with the backward planes)
        c->smem_hvp = sizeof(float) * (size_t)std::max(chain_layout(dims->hidden1 / 16, dims->hidden2 / 16, CHAIN_NW_HVP, true, c->NP).total,
                                                       chain_layout(dims->hidden1 / 16, dims->hidden2 / 16, CHAIN_NW_HVP, true, c->NP, true).total);
        break;
    }
    if (c->smem_hvp > 160 * 1024 || c->smem_fwd > 160 * 1024) {
        const size_t need = c->smem_hvp > c->smem_fwd ? c->smem_hvp : c->smem_fwd;
        return fail(-1, "LDS budget exceeded (%zu bytes)", need);
    }
    {   // dynamic LDS past the default limit, for every instance of every family
        const int lds = 160 * 1024;
#define PROMP_CHAIN_LDS(N1, N2, KS) if (allow_lds(lds, k_chain_hvp<N1, N2, KS, CHAIN_NW_HVP, false>, k_chain_hvp<N1, N2, KS, CHAIN_NW_HVP, true>)) return -2;
        PROMP_CHAIN_ALL(PROMP_CHAIN_LDS)
#undef PROMP_CHAIN_LDS
#define PROMP_PASS_LDS(N1, N2) \
    if (allow_lds(lds, k_pass<N1, N2, CHAIN_NW_HVP, true, true>, k_pass<N1, N2, CHAIN_NW_HVP, true, false>, k_pass<N1, N2, CHAIN_NW_HVP, false, false>)) return -2;
        PROMP_PASS_ALL(PROMP_PASS_LDS)
#undef PROMP_PASS_LDS
#define PROMP_WB_LDS(CLS, NKO, NXB) if (allow_lds(lds, k_wb_hvp<NKO, NXB>, k_wb_fwd_bwd<NKO, NXB, true>, k_wb_fwd_bwd<NKO, NXB, false>)) return -2;
        PROMP_WB_ALL(PROMP_WB_LDS)
#undef PROMP_WB_LDS
#define PROMP_WIDE_LDS(HH, NOB) if (allow_lds(lds, k_wide_fwd_bwd<HH, NOB, true>, k_wide_fwd_bwd<HH, NOB, false>, k_wide_hvp<HH, NOB>)) return -2;
        PROMP_WIDE_ALL(PROMP_WIDE_LDS)
#undef PROMP_WIDE_LDS
#define PROMP_GEN_LDS(NBW)                                                                                                   \
    if (allow_lds(lds, k_gen_linear<GEN_FWD, NBW>, k_gen_linear<GEN_FWD_T, NBW>, k_gen_linear<GEN_BWD, NBW>, k_gen_linear<GEN_BWD_T, NBW>, \
                  k_gen_wgrad<1, NBW>, k_gen_wgrad<2, NBW>, k_gb_linear<GEN_FWD, NBW>, k_gb_linear<GEN_FWD_T, NBW>,            \
                  k_gb_linear<GEN_BWD, NBW>, k_gb_linear<GEN_BWD_T, NBW>, k_gb_wgrad<1, NBW>, k_gb_wgrad<2, NBW>)) return -2;
        PROMP_GEN_LDS(1) PROMP_GEN_LDS(2) PROMP_GEN_LDS(3) PROMP_GEN_LDS(4)
#undef PROMP_GEN_LDS
        if (allow_lds((int)gen_loss_smem(GEN_MAX_A), k_gen_loss<true, true>, k_gen_loss<false, true>, k_gen_loss<false, false>)) return -2;
#define PROMP_GRAM_INST(NBLK) k_gram<NBLK>,
#define PROMP_FITWV_INST(DT) k_fit_wave<DT>,
        if (allow_lds(lds, PROMP_GRAM_ALL(PROMP_GRAM_INST) PROMP_FITWV_ALL(PROMP_FITWV_INST) k_fit, k_gram_wide, k_gram_tiled<GRAMT_TB, GRAMT_NWV, GRAMT_NLD>, k_fitw_panel<32>, k_fitw_panel<16>,
                      k_fitw_update<32>, k_fitw_update<16>, k_fitw_back<32>, k_fitw_back<16>, k_fit_wide<32>, k_fit_wide<16>)) return -2;
#undef PROMP_GRAM_INST
#undef PROMP_FITWV_INST
    }
    const size_t NP = c->NP, MNP = (size_t)M * NP;
    if (c->theta.alloc(NP) || c->step_sizes.alloc(NP)) return -2;
    if (c->adam_m.alloc(NP) || c->adam_v.alloc(NP)) return -2;
    if (c->theta_tasks.alloc(MNP) || c->chain.alloc((size_t)(K + 1) * MNP)) return -2;
    if (c->lam.alloc(MNP) || c->vbuf.alloc(MNP)) return -2;
    if (c->family == PassFamily::CoopSplit) {
        const size_t pw = (size_t)M * wb_planes_words(wb_nko(c->wb_cls));
        if (c->wb_planes.alloc(pw) || c->wb_vplanes.alloc(pw) || c->wb_planes_meta.alloc(pw)) return -2;
        if (c->vdir_absmax.alloc((size_t)M)) return -2;
    }
    if (c->partials.alloc((size_t)c->max_work * c->partial_stride)) return -2;
    if (c->scal_inner.alloc((size_t)K * M * 2) || c->scal_outer.alloc((size_t)M * 2)) return -2;
    if (c->scal_tmp.alloc((size_t)M * 2)) return -2;
    if (c->red.alloc(final_red_count(NP, K, false)) || c->grad_mean.alloc(NP)) return -2;
    if (c->stats.alloc((size_t)2 * (K + 2))) return -2;
    // (the baseline fit's partial Gram blocks and scratch matrices -- 2.7 GB per set at Humanoid's 757 columns -- are allocated by the
    //  first promp_process_samples that fits a baseline on that stream: fit_buffers())
    if (c->red64.alloc(64)) return -2;
    if (c->family == PassFamily::Layered) {
        const size_t R = (size_t)dims->max_rows;
        for (int l = 1; l < c->n_lin; ++l)
            if (c->g_act[l].alloc(R * c->lin[l].K) || c->g_ract[l].alloc(R * c->lin[l].K)) return -2;
        if (c->g_mu.alloc(R * dims->act_dim) || c->g_rmu.alloc(R * dims->act_dim)) return -2;
        for (int i = 0; i < 2; ++i)
            if (c->g_dz[i].alloc(R * c->g_maxw) || c->g_qz[i].alloc(R * c->g_maxw)) return -2;
        if (c->gen_bf16 && (c->gb_wplanes.alloc((size_t)M * c->gb_plane_stride) || c->gb_vplanes.alloc((size_t)M * c->gb_plane_stride))) return -2;
    }
    if (c->task_counters.alloc((size_t)M)) return -2;
    if (c->dbg.alloc(256 + 4 * 1024)) return -2;
    if (c->split_events.alloc(4)) return -2;
    if (c->stats_host.alloc(2 * (K + 2) + 1)) return -2;
    if (c->stats_seq_host.alloc(1)) return -2;
    *c->stats_seq_host = 0;
    c->steps.resize(K + 1);
    for (auto& S : c->steps)
        if (alloc_step(c, S)) return -2;
    *out = guard.release();
    return 0;
}

// (delete releases what the context's members own, in reverse order of declaration: buffers and events first, the streams last)
void promp_ctx_destroy(promp_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->copy) (void)hipStreamSynchronize(c->copy);
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) ncclCommDestroy(c->comm);
    delete c;
}

int promp_sync(promp_ctx* c) {
    NEED_CTX(c);
    if (c->copy) HIPCHECK(hipStreamSynchronize(c->copy));
    HIPCHECK(hipStreamSynchronize(c->side));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// Offsets, time indices and the three work tables of one sampling step (everything of promp_upload_step but the data), built by
// build_step_tables (promp_plan.h).
// `S` is the slab set to describe and `st` the stream the table copies go to: the step's current set on the main stream
// (promp_upload_step; synchronous), or its back set on the copy stream (promp_stage_step; the host-side tables are
// then kept alive in S.host_tables until the set is staged again).
static int set_step_layout(promp_ctx* c, StepData& S, hipStream_t st, bool async, int n_paths, const int32_t* tpo, const int32_t* pro) {
    if (!tpo || !pro) return fail(-1, "offsets are required");
    const int M = c->d.n_tasks;
    S.ps.obs_range_valid = false;         // (whoever describes a slab anew is about to fill it)
    // Same offsets as the batch this set held before (fixed-horizon environments: every batch): the time indices and the
    // work tables on the device are already the right ones -- nothing to rebuild on the host (0.3 ms at 160 000 rows), no
    // table copies to enqueue.  (A set is only ever re-described after its previous table copies have completed.)
    // (A match also means the offsets are well-formed: the set was built from them.)
    if ((int)S.lay_tpo.size() == M + 1 && (int)S.lay_pro.size() == n_paths + 1 && S.n_paths == n_paths &&
        memcmp(S.lay_tpo.data(), tpo, sizeof(int) * (M + 1)) == 0 && memcmp(S.lay_pro.data(), pro, sizeof(int) * (n_paths + 1)) == 0) {
        S.processed = false; S.has_adv = false; S.has_rew64 = false; S.has_dice = false; S.dice_processed = false; S.has_dice_vpg = false;
        return 0;
    }
    // every source of the copies below lives in `keep` (asynchronous mode: until the set is staged again)
    auto keep = std::make_shared<StepTables>();
    std::string why;
    if (const int rc = build_step_tables(c->n_cus, c->max_work, c->d.max_rows, c->d.max_paths, M, n_paths, tpo, pro, keep.get(), &why))
        return fail_plan(rc, why);
    const StepTables& k = *keep;
    const int R = (int)k.row_t.size();
    S.lay_tpo.clear(); S.lay_pro.clear();         // (set again at the end; stays empty if a copy fails half-way)
    S.n_paths = n_paths; S.n_rows = R; S.n_work[0] = (int)k.work[0].size(); S.n_work[1] = (int)k.work[1].size();
    S.processed = false; S.has_adv = false; S.has_rew64 = false; S.has_dice = false; S.dice_processed = false; S.has_dice_vpg = false;
    HIPCHECK(hipMemcpyAsync(S.path_row_offsets, k.pro.data(), sizeof(int) * (n_paths + 1), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(S.task_path_offsets, k.tpo.data(), sizeof(int) * (M + 1), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(S.path_task, k.path_task.data(), sizeof(int) * n_paths, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(S.row_t, k.row_t.data(), sizeof(int) * R, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(S.task_row_offsets, k.tro.data(), sizeof(int) * (M + 1), hipMemcpyHostToDevice, st));
    S.n_chain_wg = (int)k.wg_off.size() - 1;
    HIPCHECK(hipMemcpyAsync(S.chain_segs, k.segs.data(), sizeof(ChainSeg) * k.segs.size(), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(S.chain_wg_offsets, k.wg_off.data(), sizeof(int) * k.wg_off.size(), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(S.chain_slot_offsets, k.slot_chain.data(), sizeof(int) * (M + 1), hipMemcpyHostToDevice, st));
    for (int t = 0; t < 2; ++t) {
        HIPCHECK(hipMemcpyAsync(S.task_wg_offsets[t], k.two[t].data(), sizeof(int) * (M + 1), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(S.work[t], k.work[t].data(), sizeof(WorkItem) * k.work[t].size(), hipMemcpyHostToDevice, st));
    }
    if (async) S.host_tables = keep;
    else HIPCHECK(hipStreamSynchronize(st));  // the sources go out of scope
    S.lay_tpo.assign(tpo, tpo + M + 1);
    S.lay_pro.assign(pro, pro + n_paths + 1);
    return 0;
}

static int copy_step_data(promp_ctx* c, StepData& S, hipStream_t st, const float* obs, const float* act, const float* rew,
                          const float* old_mean, const float* old_ls, int ls_per_row,
                          hipMemcpyKind kind = hipMemcpyHostToDevice) {   // (promp_upload_step_dev: the sources are device memory)
    const int M = c->d.n_tasks;
    const size_t R = (size_t)S.n_rows;
    const size_t O = c->d.obs_dim, A = c->d.act_dim;
    HIPCHECK(hipMemcpyAsync(S.obs, obs, sizeof(float) * R * O, kind, st));
    if (enqueue_obs_range(c, pass_slab(S), st)) return -2;
    HIPCHECK(hipMemcpyAsync(S.rew, rew, sizeof(float) * R, kind, st));
    S.has_policy = act && old_mean && old_ls;
    if (S.has_policy) {
        S.ls_per_row = ls_per_row ? 1 : 0;
        HIPCHECK(hipMemcpyAsync(S.act, act, sizeof(float) * R * A, kind, st));
        HIPCHECK(hipMemcpyAsync(S.old_mean, old_mean, sizeof(float) * R * A, kind, st));
        HIPCHECK(hipMemcpyAsync(S.old_ls, old_ls, sizeof(float) * (ls_per_row ? (size_t)R : (size_t)M) * A, kind, st));
    }
    return 0;
}

int promp_upload_step(promp_ctx* c, int step, int n_paths, const int32_t* tpo, const int32_t* pro, const float* obs,
                      const float* act, const float* rew, const float* old_mean, const float* old_ls, int ls_per_row) {
    if (c && (!obs || !rew)) return fail(-1, "offsets, obs and rew are required");
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    clear_selection(c, step);
    if (set_step_layout(c, S, c->stream, false, n_paths, tpo, pro)) return -2;
    return copy_step_data(c, S, c->stream, obs, act, rew, old_mean, old_ls, ls_per_row);
}

// ---- staged uploads: the NEXT batch travels while the current one is computed ------------------------------------------
void* promp_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail(-2, "hipHostMalloc of %zu bytes failed", bytes);
        return nullptr;
    }
    return p;
}
void promp_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int promp_stage_step(promp_ctx* c, int step, int n_paths, const int32_t* tpo, const int32_t* pro, const float* obs,
                     const float* act, const float* rew, const float* old_mean, const float* old_ls, int ls_per_row) {
    NEED_CTX(c);
    if (!obs || !rew) return fail(-1, "offsets, obs and rew are required");
    if (step < 0 || step > c->d.num_inner_steps) return fail(-1, "step %d out of range", step);
    if (!c->copy) HIPCHECK(hipStreamCreate(&c->copy.h));
    if (c->back.empty()) {
        c->back.resize(c->steps.size());
        for (auto& B : c->back)
            if (alloc_step(c, B)) return -2;
    }
    StepData& B = c->back[step];
    // the set's previous life: host tables of its last staging, and whatever the compute streams still read from it
    if (B.ready_set) HIPCHECK(hipEventSynchronize(B.ev_ready));
    if (mark_use(c, B)) return -2;           // (normally settled already by the entry points that came after its last use)
    if (B.use_set) HIPCHECK(hipStreamWaitEvent(c->copy, B.ev_use, 0));
    if (B.side_pending) {
        HIPCHECK(hipStreamWaitEvent(c->copy, B.ev_done, 0));
        B.side_pending = false;
    }
    if (set_step_layout(c, B, c->copy, true, n_paths, tpo, pro)) return -2;
    if (copy_step_data(c, B, c->copy, obs, act, rew, old_mean, old_ls, ls_per_row)) return -2;
    HIPCHECK(hipEventRecord(B.ev_ready, c->copy));
    B.ready_set = true;
    B.wait_ready_main = B.wait_ready_side = true;
    B.staged = true;
    return 0;
}

int promp_commit_step(promp_ctx* c, int step) {
    NEED_CTX(c);
    if (step < 0 || step > c->d.num_inner_steps) return fail(-1, "step %d out of range", step);
    if (c->back.empty() || !c->back[step].staged) return fail(-3, "step %d has nothing staged", step);
    // uses of the outgoing set that are still unmarked get their mark now, while "everything enqueued so far" is tight
    if (mark_use(c, c->steps[step])) return -2;
    clear_selection(c, step);
    std::swap(c->steps[step], c->back[step]);
    c->steps[step].staged = false;
    c->steps[step].data_version = ++c->version_counter;
    return 0;
}

int promp_stage_wait(promp_ctx* c) {
    NEED_CTX(c);
    if (c->copy) HIPCHECK(hipStreamSynchronize(c->copy));
    return 0;
}

// The baseline fit's buffers of one stream (main / side), allocated on first use: contexts that never fit a LinearFeatureBaseline
// (policy passes only, ZeroBaseline, advantages handed in) do not pay for them.
int fit_buffers(promp_ctx* c, bool on_side, const SamplePlan& plan) {
    DevBuf<double>& gp = on_side ? c->gram_partials_side : c->gram_partials;
    DevBuf<double>& fs = on_side ? c->fit_scratch_side : c->fit_scratch;
    if (!gp && gp.alloc((size_t)c->max_work * c->gram_stride)) return -2;
    if (!fs && plan.fit == FitKernel::Wide && fs.alloc((size_t)c->d.n_tasks * 2 * (c->Dmax + 1) * (c->Dmax + 1) + c->d.n_tasks)) return -2;   // (+ k_fitw_back's flags)
    return 0;
}

// What every sample kernel reads of a step (promp_predict_baseline's k_gae needs no more); everything else is zero and the caller
// sets what its kernels use
static SampleArgs sample_args(const promp_ctx* c, const StepData& S, int kind) {
    SampleArgs a;
    memset(&a, 0, sizeof a);
    a.obs = S.obs; a.rew = S.rew; a.rew64 = S.has_rew64 ? S.rew64.p : nullptr; a.path_row_offsets = S.path_row_offsets; a.path_task = S.path_task; a.row_t = S.row_t;
    a.task_row_offsets = S.task_row_offsets; a.task_path_offsets = S.task_path_offsets;
    a.O = c->d.obs_dim; a.kind = kind; a.D = feature_dim(&c->d, kind);
    a.adv64 = S.adv64; a.path_mom = S.path_mom; a.coeffs = S.coeffs; a.coeff_stride = c->coeff_stride;
    return a;
}

// Where a step's sample processing runs.  Steps >= 1 go to the second stream (no data dependence on the step-0 work the host
// enqueued just before: their samples are resident), behind the last main-stream work that touched this step's slabs.  Per-kernel
// timing (promp_profile) keeps everything on the one stream it brackets.
struct SampleStream {
    bool on_side = false;
    hipStream_t st = nullptr;
    double* gram_partials = nullptr;
    double* fit_scratch = nullptr;
};
// the prologue promp_process_samples and promp_process_samples_dice share: the stream, the fit's buffers for every plan the call
// launches, the event waits
static int sample_stream_begin(promp_ctx* c, int step, StepData& S, std::initializer_list<const SamplePlan*> plans, SampleStream* ss) {
    ss->on_side = c->overlap && !c->prof && step >= 1;
    ss->st = ss->on_side ? c->side : c->stream;
    for (const SamplePlan* plan : plans)
        if (plan->gram != GramKernel::None && fit_buffers(c, ss->on_side, *plan)) return -2;
    ss->gram_partials = ss->on_side ? c->gram_partials_side : c->gram_partials;
    ss->fit_scratch = ss->on_side ? c->fit_scratch_side : c->fit_scratch;
    if (ss->on_side) {
        if (mark_use(c, S)) return -2;
        if (S.use_set) HIPCHECK(hipStreamWaitEvent(c->side, S.ev_use, 0));
        if (S.wait_ready_side) HIPCHECK(hipStreamWaitEvent(c->side, S.ev_ready, 0));
    }
    S.wait_ready_side = false;
    return 0;
}
static int sample_stream_end(promp_ctx* c, StepData& S, const SampleStream& ss) {
    if (ss.on_side) {
        HIPCHECK(hipEventRecord(S.ev_done, c->side));
        S.side_pending = true;
    }
    return 0;
}

// The Gram and fit kernels sample_plan() picked, on the target in a.ret64: the task's coefficients into a.coeffs
static int launch_fit(promp_ctx* c, StepData& S, const SampleArgs& a, const SamplePlan& plan, const SampleStream& ss) {
    hipStream_t st = ss.st;
    double* fit_scratch = ss.fit_scratch;
    const int nblk = plan.nblk, DA = a.D + 1, M = c->d.n_tasks;
    if (plan.gram != GramKernel::None && prof_begin(c, PROMP_KERNEL_GRAM, S.n_rows)) return -2;
    switch (plan.gram) {
    case GramKernel::None: break;
    case GramKernel::Small:
        switch (plan.gram_nblk) {
#define PROMP_GRAM_CASE(NBLK) \
    case NBLK: { auto k = k_gram<NBLK>; PROMP_LAUNCH(k, dim3(S.n_work[0]), 64 * GramCfg<NBLK>::NW, GramCfg<NBLK>::SMEM_BYTES, st, a); } break;
            PROMP_GRAM_ALL(PROMP_GRAM_CASE)
#undef PROMP_GRAM_CASE
        }
        break;
    case GramKernel::Tiled: {
        if (c->gramt_map_nblk != nblk) { gramt_balance(nblk, GRAMT_NWV, &c->gramt_map); c->gramt_map_nblk = nblk; }
        auto k = k_gram_tiled<GRAMT_TB, GRAMT_NWV, GRAMT_NLD>;
        PROMP_LAUNCH(k, dim3(S.n_work[0], plan.gram_slices), 64 * GRAMT_NWV, gramt_smem(nblk, plan.gram_rows, plan.gram_db), st, a, nblk,
                     c->gramt_map, plan.gram_rows, plan.gram_db);
        break;
    }
    case GramKernel::Wide:
        PROMP_LAUNCH(k_gram_wide, dim3(S.n_work[0], plan.gram_slices), 512, gramw_smem(nblk, a.O, plan.gram_rows), st, a, nblk, plan.gram_rows);
        break;
    }
    HIPCHECK(hipGetLastError());
    if (plan.gram != GramKernel::None && prof_end(c, PROMP_KERNEL_GRAM)) return -2;
    const size_t fit_smem = sizeof(double) * ((size_t)2 * DA * DA + 3 * DA + 2 + fitwv_aux(64));      // (k_fit / k_fit_wave<DT <= 64>)
    switch (plan.fit) {
    case FitKernel::None: break;
    case FitKernel::Wave:
        switch (plan.fit_arg) {
#define PROMP_FITWV_CASE(DT) case DT: { auto k = k_fit_wave<DT>; PROMP_LAUNCH(k, dim3(M), FITWV_NT, fit_smem, st, a, nblk); } break;
            PROMP_FITWV_ALL(PROMP_FITWV_CASE)
#undef PROMP_FITWV_CASE
        }
        break;
    case FitKernel::Block: PROMP_LAUNCH(k_fit, dim3(M), 256, fit_smem, st, a, nblk); break;
    case FitKernel::Wide: {
        PROMP_LAUNCH(k_gram_sum_wide, dim3(M * plan.sum_split), 256, 0, st, a, nblk, fit_scratch, plan.sum_split);
        HIPCHECK(hipGetLastError());
        const int* none = nullptr;
        int* bad = (int*)(fit_scratch + (size_t)M * 2 * (c->Dmax + 1) * (c->Dmax + 1));
#define PROMP_FITW(NB)                                                                                                              \
    if (plan.fit_phases) {                                                                                                          \
        auto kp = k_fitw_panel<NB>; auto ku = k_fitw_update<NB>; auto kb = k_fitw_back<NB>; auto kf = k_fit_wide<NB>;              \
        for (int k0 = 0; k0 < a.D; k0 += NB) {                                                                                      \
            PROMP_LAUNCH(kp, dim3(M), FITW_NT, fitw_panel_smem(a.D, NB), st, a, fit_scratch, k0);                                   \
            if (k0 + NB < a.D) PROMP_LAUNCH(ku, dim3(M, FITW_UPD_SPLIT), FITW_NT, fitw_panel_smem(a.D, NB), st, a, fit_scratch, k0); \
        }                                                                                                                           \
        PROMP_LAUNCH(kb, dim3(M), FITW_NT, fitw_back_smem(a.D, NB), st, a, fit_scratch, bad);                                       \
        PROMP_LAUNCH(kf, dim3(M), FITW_NT, fitw_smem(a.D, NB), st, a, nblk, fit_scratch, (const int*)bad);                          \
    } else { auto k = k_fit_wide<NB>; PROMP_LAUNCH(k, dim3(M), FITW_NT, fitw_smem(a.D, NB), st, a, nblk, fit_scratch, none); }
        switch (plan.fit_arg) {
        case 32: PROMP_FITW(32) break;
        case 16: PROMP_FITW(16) break;
        }
#undef PROMP_FITW
        break;
    }
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// what promp_process_samples and promp_process_samples_dice hand their kernels: the step's arrays, the call's options
static SampleArgs process_args(const promp_ctx* c, const StepData& S, const SampleStream& ss, int kind, double discount, double gae_lambda,
                               double reg_coeff, int normalize_adv, int positive_adv) {
    SampleArgs a = sample_args(c, S, kind);
    a.work = S.work[0];                         // k_gram / k_fit: one workgroup per CU
    a.task_wg_offsets = S.task_wg_offsets[0];
    a.gamma = discount; a.lam = gae_lambda; a.reg = reg_coeff;
    a.normalize = normalize_adv; a.positive = positive_adv;
    a.ret64 = S.ret64; a.ret32 = S.ret32; a.adv32 = S.adv32;
    a.path_ret0 = S.path_ret0; a.path_undisc = S.path_undisc; a.path_rsq = S.path_rsq;
    a.gram_partials = ss.gram_partials;
    return a;
}
// returns -> fit -> GAE -> normalise (a.work moves on to the second table for k_normalize)
static int launch_gae_pipeline(promp_ctx* c, StepData& S, SampleArgs& a, const SamplePlan& plan, const SampleStream& ss) {
    hipStream_t st = ss.st;
    PROMP_LAUNCH(k_returns, dim3(S.n_paths), 64, 0, st, a);
    HIPCHECK(hipGetLastError());
    if (const int rc = launch_fit(c, S, a, plan, ss)) return rc;
    PROMP_LAUNCH(k_gae, dim3(S.n_paths), 64, sizeof(double) * (size_t)(a.D > 0 ? a.D : 1), st, a);
    HIPCHECK(hipGetLastError());
    a.work = S.work[1];                         // k_normalize: two workgroups per CU
    PROMP_LAUNCH(k_normalize, dim3(S.n_work[1]), 256, 0, st, a);
    HIPCHECK(hipGetLastError());
    return 0;
}

int promp_process_samples(promp_ctx* c, int step, const promp_proc_opts* o) {
    if (!c || !o) return fail(-1, "NULL argument");
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/true);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (!(o->discount >= 0 && o->discount <= 1)) return fail(-1, "discount factor must be in [0,1]");      // samplers/base.py:57
    if (!(o->gae_lambda >= 0 && o->gae_lambda <= 1)) return fail(-1, "gae_lambda must be in [0,1]");       // samplers/base.py:58
    if (o->baseline_kind < 0 || o->baseline_kind > 2) return fail(-1, "unknown baseline kind %d", o->baseline_kind);
    if (o->reserved < 0) return fail(-1, "pad_length %d is negative", o->reserved);
    // which Gram and fit kernels run (promp_plan.h: sample_plan; the table in tests/test_gpu_parity.py)
    SamplePlan plan;
    std::string why;
    if (const int rc = sample_plan(o->baseline_kind, c->d.obs_dim, feature_dim(&c->d, o->baseline_kind), c->sw, &plan, &why))
        return fail_plan(rc, why);
    SampleStream ss;
    if (const int rc = sample_stream_begin(c, step, S, {&plan}, &ss)) return rc;
    SampleArgs a = process_args(c, S, ss, o->baseline_kind, o->discount, o->gae_lambda, o->reg_coeff, o->normalize_adv, o->positive_adv);
    a.pad_length = o->reserved;                 // non-zero: the statistics of the zero-padded [paths, pad_length] array
    S.feat_dim = a.D;
    if (const int rc = launch_gae_pipeline(c, S, a, plan, ss)) return rc;
    if (const int rc = sample_stream_end(c, S, ss)) return rc;
    S.processed = true;
    S.has_adv = true;
    S.dice_processed = false;
    return 0;
}

int promp_download_processed(promp_ctx* c, int step, float* returns, float* adv, double* coeffs, double* ret0,
                             double* undisc, double* rsq) {
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (!S.processed) return fail(-3, "step %d has not been processed", step);
    hipStream_t st = c->stream;
    if (returns) HIPCHECK(hipMemcpyAsync(returns, S.ret32, sizeof(float) * S.n_rows, hipMemcpyDeviceToHost, st));
    if (adv) HIPCHECK(hipMemcpyAsync(adv, S.adv32, sizeof(float) * S.n_rows, hipMemcpyDeviceToHost, st));
    // the small results (three per-path sums, the tasks' coefficients) land in one page-locked staging area behind ONE
    // synchronisation and are copied out from there: the caller's arrays are pageable, and a device-to-pageable copy is a
    // synchronous bounce each (the plugin classes make this call once per sampling step)
    const size_t P = (size_t)S.n_paths, NC = (coeffs && S.feat_dim > 0) ? (size_t)c->d.n_tasks * c->coeff_stride : 0;
    if (c->small_host.reserve(3 * P + NC, 1)) return -2;
    double* h = c->small_host;
    if (ret0) HIPCHECK(hipMemcpyAsync(h, S.path_ret0, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    if (undisc) HIPCHECK(hipMemcpyAsync(h + P, S.path_undisc, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    if (rsq) HIPCHECK(hipMemcpyAsync(h + 2 * P, S.path_rsq, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    if (NC) HIPCHECK(hipMemcpyAsync(h + 3 * P, S.coeffs, sizeof(double) * NC, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (ret0) memcpy(ret0, h, sizeof(double) * P);
    if (undisc) memcpy(undisc, h + P, sizeof(double) * P);
    if (rsq) memcpy(rsq, h + 2 * P, sizeof(double) * P);
    if (NC)
        for (int i = 0; i < c->d.n_tasks; ++i)
            memcpy(coeffs + (size_t)i * S.feat_dim, h + 3 * P + (size_t)i * c->coeff_stride, sizeof(double) * S.feat_dim);
    return 0;
}

int promp_download_raw(promp_ctx* c, int step, double* ret64, double* adv64) {
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (!S.processed) return fail(-3, "step %d has not been processed", step);
    if (ret64) HIPCHECK(hipMemcpyAsync(ret64, S.ret64, sizeof(double) * S.n_rows, hipMemcpyDeviceToHost, c->stream));
    if (adv64) HIPCHECK(hipMemcpyAsync(adv64, S.adv64, sizeof(double) * S.n_rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int promp_set_coeffs(promp_ctx* c, int step, int kind, const double* coeffs) {
    if (!c || !coeffs) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (kind < 1 || kind > 2) return fail(-1, "coefficients exist for the linear baselines only");
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    StepData& S = sc.S();
    const int D = feature_dim(&c->d, kind), M = c->d.n_tasks;
    std::vector<double> tmp((size_t)M * c->coeff_stride, 0.0);
    for (int i = 0; i < M; ++i) memcpy(tmp.data() + (size_t)i * c->coeff_stride, coeffs + (size_t)i * D, sizeof(double) * D);
    HIPCHECK(hipMemcpyAsync(S.coeffs, tmp.data(), sizeof(double) * tmp.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    S.feat_dim = D;
    return 0;
}

int promp_predict_baseline(promp_ctx* c, int step, int kind, double* out) {
    if (!c || !out) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (kind < 0 || kind > 2) return fail(-1, "unknown baseline kind %d", kind);
    if (sc.open(/*writes=*/false, /*needs_data=*/true)) return sc.rc;
    StepData& S = sc.S();
    SampleArgs a = sample_args(c, S, kind);
    a.gamma = 1.0; a.lam = 1.0;
    a.bl64 = S.ret64;                              // scratch: returns of this step are recomputed by process_samples
    if (kind == PROMP_BASELINE_ZERO) HIPCHECK(hipMemsetAsync(S.ret64, 0, sizeof(double) * S.n_rows, c->stream));
    PROMP_LAUNCH(k_gae, dim3(S.n_paths), 64, sizeof(double) * (size_t)(a.D > 0 ? a.D : 1), c->stream, a);
    HIPCHECK(hipGetLastError());
    S.processed = false;
    S.has_adv = false;
    HIPCHECK(hipMemcpyAsync(out, S.ret64, sizeof(double) * S.n_rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int promp_set_advantages(promp_ctx* c, int step, const float* adv) {
    if (!c || !adv) return fail(-1, "NULL argument");
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/true);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    HIPCHECK(hipMemcpyAsync(S.adv32, adv, sizeof(float) * S.n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    S.has_adv = true;
    return 0;
}

int promp_set_step_selection(promp_ctx* c, int step, int n_sel, const int32_t* path_idx) {
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (n_sel < 0) return fail(-1, "n_sel %d is negative", n_sel);
    if (n_sel == 0 || !path_idx) {
        if ((size_t)step < c->sel.size() && c->sel[step].on) {
            clear_selection(c, step);
            ++c->version_counter;
        }
        return 0;
    }
    const StepData& P = sc.S();
    const int M = c->d.n_tasks, K = c->d.num_inner_steps;
    if (P.n_rows == 0 || (int)P.lay_tpo.size() != M + 1) return fail(-3, "step %d has no data", step);
    // everything that can refuse comes first: the selection, the compact slab's tables, the buffers every selection shares
    SelectionLayout lay;
    StepTables tables;
    std::string why;
    if (const int rc = build_selection(M, P.n_paths, P.lay_tpo.data(), P.lay_pro.data(), n_sel, path_idx, &lay, &why)) return fail_plan(rc, why);
    if (const int rc = build_step_tables(c->n_cus, c->max_work, lay.pro[n_sel], n_sel, M, n_sel, lay.tpo.data(), lay.pro.data(), &tables, &why))
        return fail_plan(rc, why);
    // the table block of the one copy launch that fills the compact slab: the selection as a partition with B = 1
    const TableBlock blk(P.n_paths, 1, M, c->max_work);
    std::vector<int> image(blk.total);
    pack_table_block(blk, selection_copy_table(P.n_paths, lay), {0}, &tables, image.data());
    if (c->sel.empty()) {
        const size_t MNP = (size_t)M * c->NP;
        if (c->sel_chain.alloc((size_t)(K + 1) * MNP) || c->sel_scal_inner.alloc((size_t)K * M * 2)) return -2;
        c->sub.resize(K + 1);
        c->sel.resize(K + 1);
    }
    Selection& L = c->sel[step];
    L.on = true; L.lay = std::move(lay); L.tables = std::move(tables); L.image = std::move(image);
    L.gathered = false;
    c->chvp_sel.valid = false;             // (its caches hold another selection's rows)
    ++c->version_counter;
    return 0;
}

int promp_step_selection(promp_ctx* c, int step) {
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    return ((size_t)step < c->sel.size() && c->sel[step].on) ? (int)c->sel[step].lay.idx.size() : 0;
}

int promp_use_selection(promp_ctx* c, int on) {
    NEED_CTX(c);
    c->use_sel = on != 0;
    return 0;
}

// The step's DiCE buffers, allocated on first use: the four of the objective (promp_set_dice_rewards and
// promp_process_samples_dice) and, processing, what promp_process_samples_dice keeps beside them
static int dice_buffers(promp_ctx* c, StepData& S, bool processing) {
    const size_t R = c->d.max_rows, P = c->d.max_paths, M = c->d.n_tasks;
    // (dice_rw / dice_path last: the guards stand for their groups)
    if (!S.dice_rw && (S.dice_c.alloc(R) || S.dice_u.alloc(R) || S.dice_tmp.alloc(R) || S.dice_rw.alloc(R))) return -2;
    if (processing && !S.dice_path &&
        (S.dice_x64.alloc(R) || S.dice_adv64.alloc(R) || S.dice_vpg32.alloc(R) || S.dice_pad.alloc(2 * M) ||
         S.dice_coeffs.alloc(M * c->coeff_stride) || S.dice_path.alloc(3 * P)))
        return -2;
    return 0;
}

int promp_set_dice_rewards(promp_ctx* c, int step, const float* rw) {
    if (!c || !rw) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (sc.open(/*writes=*/true, /*needs_data=*/true)) return sc.rc;
    StepData& S = sc.S();
    if (dice_buffers(c, S, /*processing=*/false)) return -2;
    S.dice_processed = false;
    S.has_dice_vpg = false;
    HIPCHECK(hipMemcpyAsync(S.dice_rw, rw, sizeof(float) * S.n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));      // (the source may be a temporary of the caller)
    // the gradient weights w_t = sum_{t' >= t} rw_t' take the advantages' place in the log-likelihood objective
    DiceScanArgs ds;
    ds.path_row_offsets = S.path_row_offsets; ds.rw = S.dice_rw; ds.c = nullptr; ds.out = S.adv32; ds.tmp = nullptr; ds.mode = 0;
    PROMP_LAUNCH(k_dice_scan, dim3(S.n_paths), 64, 0, c->stream, ds);
    HIPCHECK(hipGetLastError());
    S.has_adv = true;
    S.has_dice = true;
    return 0;
}

int promp_process_samples_dice(promp_ctx* c, int step, const promp_dice_opts* o) {
    if (!c || !o) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (!(o->discount >= 0 && o->discount <= 1)) return fail(-1, "discount factor must be in [0,1]");      // dice_sample_processor.py:38
    if (!(o->gae_lambda >= 0 && o->gae_lambda <= 1)) return fail(-1, "gae_lambda must be in [0,1]");
    if (o->baseline_kind < 0 || o->baseline_kind > 2) return fail(-1, "unknown baseline kind %d", o->baseline_kind);
    const bool vpg = o->return_baseline_kind != -1;
    if (vpg && (o->return_baseline_kind < 0 || o->return_baseline_kind > 2)) return fail(-1, "unknown return baseline kind %d", o->return_baseline_kind);
    if (sc.open(/*writes=*/true, /*needs_data=*/true)) return sc.rc;
    StepData& S = sc.S();
    if ((int)S.lay_pro.size() != S.n_paths + 1) return fail(-3, "step %d has no data", step);
    int longest = 0;
    for (int p = 0; p < S.n_paths; ++p) longest = std::max(longest, S.lay_pro[p + 1] - S.lay_pro[p]);
    if (o->max_path_length < longest)
        return fail(-1, "max_path_length %d is shorter than the step's longest path (%d rows)", o->max_path_length, longest);
    SamplePlan plan, rplan;
    std::string why;
    if (const int rc = sample_plan(o->baseline_kind, c->d.obs_dim, feature_dim(&c->d, o->baseline_kind), c->sw, &plan, &why)) return fail_plan(rc, why);
    if (vpg)
        if (const int rc = sample_plan(o->return_baseline_kind, c->d.obs_dim, feature_dim(&c->d, o->return_baseline_kind), c->sw, &rplan, &why))
            return fail_plan(rc, why);
    if (dice_buffers(c, S, /*processing=*/true)) return -2;
    SampleStream ss;
    if (const int rc = sample_stream_begin(c, step, S, {&plan, &rplan}, &ss)) return rc;
    hipStream_t st = ss.st;
    const int M = c->d.n_tasks, P = c->d.max_paths;
    S.processed = false; S.has_adv = false; S.has_dice = false; S.dice_processed = false; S.has_dice_vpg = false;
    // the DiCE rewards: targets -> fit -> adjust -> finish.  The reward baseline's coefficients and the path sums have places of
    // their own: the pass below overwrites the step's.
    SampleArgs a = process_args(c, S, ss, o->baseline_kind, o->discount, o->gae_lambda, o->reg_coeff, o->normalize_adv, o->positive_adv);
    a.pad_length = o->max_path_length;
    a.coeffs = S.dice_coeffs;
    a.path_undisc = S.dice_path; a.path_ret0 = S.dice_path + P; a.path_rsq = S.dice_path + 2 * (size_t)P;
    a.x64 = S.dice_x64; a.dice_rw = S.dice_rw; a.pad_out = S.dice_pad;
    PROMP_LAUNCH(k_dice_targets, dim3(S.n_paths), 64, 0, st, a);
    HIPCHECK(hipGetLastError());
    if (const int rc = launch_fit(c, S, a, plan, ss)) return rc;
    PROMP_LAUNCH(k_dice_adjust, dim3(S.n_paths), 64, sizeof(double) * (size_t)(a.D > 0 ? a.D : 1), st, a);
    HIPCHECK(hipGetLastError());
    PROMP_LAUNCH(k_dice_finish, dim3(S.n_paths), 64, 0, st, a);
    HIPCHECK(hipGetLastError());
    S.dice_feat_dim = a.D;
    S.dice_ret_feat_dim = 0;
    S.feat_dim = 0;
    if (vpg) {
        // the ordinary pipeline on the slab's true rewards, normalised over the padded array; its advantages, as slab weights,
        // beside the DiCE weights
        SampleArgs g = process_args(c, S, ss, o->return_baseline_kind, o->discount, o->gae_lambda, o->return_reg_coeff, o->normalize_adv, o->positive_adv);
        g.pad_length = o->max_path_length;
        g.pad_scale = 1;
        g.adv32 = S.dice_vpg32; g.x64 = S.dice_adv64; g.pad_out = S.dice_pad + M;
        if (const int rc = launch_gae_pipeline(c, S, g, rplan, ss)) return rc;
        S.dice_ret_feat_dim = S.feat_dim = g.D;
    }
    if (const int rc = sample_stream_end(c, S, ss)) return rc;
    S.processed = true; S.has_adv = true; S.has_dice = true; S.dice_processed = true; S.has_dice_vpg = vpg;
    return 0;
}

int promp_download_dice(promp_ctx* c, int step, double* adjusted, double* advantages, double* pad_adjusted, double* pad_advantages,
                        double* coeffs, double* return_coeffs, double* path_undisc, double* path_disc, double* path_rsq) {
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (!S.dice_processed) return fail(-3, "step %d has not been processed by promp_process_samples_dice", step);
    if ((advantages || pad_advantages || return_coeffs) && !S.has_dice_vpg)
        return fail(-3, "step %d was processed without a return baseline: it has no GAE advantages", step);
    hipStream_t st = c->stream;
    const size_t R = (size_t)S.n_rows, P = (size_t)S.n_paths, PS = (size_t)c->d.max_paths, M = (size_t)c->d.n_tasks, CS = (size_t)c->coeff_stride;
    if (adjusted) HIPCHECK(hipMemcpyAsync(adjusted, S.dice_x64, sizeof(double) * R, hipMemcpyDeviceToHost, st));
    if (advantages) HIPCHECK(hipMemcpyAsync(advantages, S.dice_adv64, sizeof(double) * R, hipMemcpyDeviceToHost, st));
    // the small results through the page-locked staging area, behind one synchronisation (as promp_download_processed)
    if (c->small_host.reserve(2 * M + 2 * M * CS + 3 * P, 1)) return -2;
    double* h = c->small_host;
    double *hpad = h, *hco = h + 2 * M, *hrco = hco + M * CS, *hpath = hrco + M * CS;
    const bool co = coeffs && S.dice_feat_dim > 0, rco = return_coeffs && S.dice_ret_feat_dim > 0;
    if (pad_adjusted || pad_advantages) HIPCHECK(hipMemcpyAsync(hpad, S.dice_pad, sizeof(double) * 2 * M, hipMemcpyDeviceToHost, st));
    if (co) HIPCHECK(hipMemcpyAsync(hco, S.dice_coeffs, sizeof(double) * M * CS, hipMemcpyDeviceToHost, st));
    if (rco) HIPCHECK(hipMemcpyAsync(hrco, S.coeffs, sizeof(double) * M * CS, hipMemcpyDeviceToHost, st));
    double* const sums[3] = {path_undisc, path_disc, path_rsq};
    for (int k = 0; k < 3; ++k)
        if (sums[k]) HIPCHECK(hipMemcpyAsync(hpath + k * P, S.dice_path + k * PS, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (pad_adjusted) memcpy(pad_adjusted, hpad, sizeof(double) * M);
    if (pad_advantages) memcpy(pad_advantages, hpad + M, sizeof(double) * M);
    for (size_t i = 0; i < M; ++i) {
        if (co) memcpy(coeffs + i * S.dice_feat_dim, hco + i * CS, sizeof(double) * S.dice_feat_dim);
        if (rco) memcpy(return_coeffs + i * S.dice_ret_feat_dim, hrco + i * CS, sizeof(double) * S.dice_ret_feat_dim);
    }
    for (int k = 0; k < 3; ++k)
        if (sums[k]) memcpy(sums[k], hpath + k * P, sizeof(double) * P);
    return 0;
}

int promp_use_dice_advantages(promp_ctx* c, int step) {
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (!sc.S().dice_processed || !sc.S().has_dice_vpg)
        return fail(-3, "step %d holds no GAE advantages: promp_process_samples_dice with a return baseline comes first", step);
    if (sc.open(/*writes=*/true, /*needs_data=*/true)) return sc.rc;
    StepData& S = sc.S();
    HIPCHECK(hipMemcpyAsync(S.adv32, S.dice_vpg32, sizeof(float) * S.n_rows, hipMemcpyDeviceToDevice, c->stream));
    S.has_adv = true;
    S.has_dice = false;      // the step's weights are advantages now: it is no longer DiCE data (vpg_dice_maml.py:46-49)
    return 0;
}

static int copy_in(promp_ctx* c, float* dst, const float* src, size_t n) {
    if (!c || !src) return fail(-1, "NULL argument");
    HIPCHECK(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
static int copy_out(promp_ctx* c, float* dst, const float* src, size_t n) {
    if (!c || !dst) return fail(-1, "NULL argument");
    HIPCHECK(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// nvec parameter vectors in the caller's layout <-> device buffers in the instantiated (zero-padded) layout
static int params_in(promp_ctx* c, float* dst, const float* src, size_t nvec) {
    if (!c || !src) return fail(-1, "NULL argument");
    if (!c->padded) return copy_in(c, dst, src, nvec * (size_t)c->NP);
    std::vector<float> tmp(nvec * (size_t)c->NP, 0.f);
    for (size_t i = 0; i < nvec; ++i) remap_params(c->du, c->d, src + i * (size_t)c->NPu, tmp.data() + i * (size_t)c->NP, true);
    return copy_in(c, dst, tmp.data(), tmp.size());
}
static int params_out(promp_ctx* c, float* dst, const float* src, size_t nvec) {
    if (!c || !dst) return fail(-1, "NULL argument");
    if (!c->padded) return copy_out(c, dst, src, nvec * (size_t)c->NP);
    std::vector<float> tmp(nvec * (size_t)c->NP);
    if (copy_out(c, tmp.data(), src, tmp.size())) return -2;
    for (size_t i = 0; i < nvec; ++i) remap_params(c->du, c->d, tmp.data() + i * (size_t)c->NP, dst + i * (size_t)c->NPu, false);
    return 0;
}

int promp_set_theta(promp_ctx* c, const float* th) {
    if (!c || !th) return fail(-1, "NULL argument");
    c->theta_version = ++c->version_counter;
    c->ls_min = th[c->NPu - c->d.act_dim];
    for (int i = 1; i < c->d.act_dim; ++i) c->ls_min = std::min(c->ls_min, th[c->NPu - c->d.act_dim + i]);
    c->ls_known = true;
    return params_in(c, c->theta, th, 1);
}
int promp_get_theta(promp_ctx* c, float* th) {
    NEED_CTX(c);
    return params_out(c, th, c->theta, 1);
}
static int mask_log_std_step_sizes(promp_ctx* c) {
    if (c->learn_std) return 0;
    HIPCHECK(hipMemsetAsync(c->step_sizes + (c->NP - c->d.act_dim), 0, sizeof(float) * c->d.act_dim, c->stream));
    return 0;
}
int promp_set_step_sizes(promp_ctx* c, const float* s) {
    NEED_CTX(c);
    c->sizes_version = ++c->version_counter;
    if (params_in(c, c->step_sizes, s, 1)) return -2;
    return mask_log_std_step_sizes(c);
}
int promp_get_step_sizes(promp_ctx* c, float* s) {
    NEED_CTX(c);
    return params_out(c, s, c->step_sizes, 1);
}
// Trainable step sizes (meta_algos/base.py:203-211,303-313).  Switching on allocates what the feature needs -- (K + 1) tasks x Theta
// floats for the inner gradients and the per-task step-size gradients, three Theta vectors, and an exchange buffer of
// 2 Theta + K + 2 floats in place of the one of Theta + K + 2 (the sums of an earlier evaluation do not survive that); switching
// off keeps the buffers and alpha's Adam slots, and every launch is again the one of a context that never had the flag on.
int promp_set_train_step_sizes(promp_ctx* c, int on) {
    NEED_CTX(c);
    if ((on != 0) == c->train_sizes) return 0;
    if (on && !c->ginner) {
        const size_t MNP = (size_t)c->d.n_tasks * c->NP;
        HIPCHECK(hipStreamSynchronize(c->stream));
        if (c->ss_grad.alloc(c->NP) || c->ss_m.alloc(c->NP) || c->ss_v.alloc(c->NP) || c->galpha.alloc(MNP)) return -2;
        {   // (into a temporary: a failed allocation leaves the context with the exchange buffer it had)
            DevBuf<float> red;
            if (red.alloc(final_red_count(c->NP, c->d.num_inner_steps, true))) return -2;
            c->red = std::move(red);
        }
        // (ginner last: the guard above stands for all six)
        if (c->ginner.alloc((size_t)c->d.num_inner_steps * MNP)) return -2;
    }
    c->train_sizes = on != 0;
    c->red_has_sizes = false;
    c->adapt0.valid = false;            // (the pass promp_inner_adapt left behind has no ginner[0] / no use for one)
    c->version_counter += 1;
    return 0;
}
int promp_get_step_size_grad(promp_ctx* c, float* out) {
    NEED_CTX(c);
    if (!c->train_sizes) return fail(-3, "the step sizes are not trained (promp_set_train_step_sizes)");
    return params_out(c, out, c->ss_grad, 1);
}
int promp_set_step_size_adam_state(promp_ctx* c, const float* m, const float* v) {
    NEED_CTX(c);
    if (!c->train_sizes) return fail(-3, "the step sizes are not trained (promp_set_train_step_sizes)");
    if (params_in(c, c->ss_m, m, 1) || params_in(c, c->ss_v, v, 1)) return -2;
    return 0;
}
int promp_get_step_size_adam_state(promp_ctx* c, float* m, float* v) {
    NEED_CTX(c);
    if (!c->train_sizes) return fail(-3, "the step sizes are not trained (promp_set_train_step_sizes)");
    if (m && params_out(c, m, c->ss_m, 1)) return -2;
    if (v && params_out(c, v, c->ss_v, 1)) return -2;
    return 0;
}
int promp_set_min_std(promp_ctx* c, float min_std) {
    NEED_CTX(c);
    if (!(min_std > 0.f)) return fail(-1, "min_std must be positive");
    c->min_log_std = logf(min_std);
    c->version_counter += 1;
    return 0;
}
int promp_set_schedule(promp_ctx* c, int stage_overlap, int fuse_min_tasks) {
    NEED_CTX(c);
    if (stage_overlap >= 0) {
        HIPCHECK(hipStreamSynchronize(c->side));
        c->overlap = stage_overlap != 0;
    }
    if (fuse_min_tasks >= 0) c->fuse_min_tasks = fuse_min_tasks;
    return 0;
}
int promp_set_reuse_adapt(promp_ctx* c, int on) {
    NEED_CTX(c);
    c->reuse_adapt = on != 0;
    c->adapt0.valid = false;
    return 0;
}
long long promp_adapt_passes_skipped(promp_ctx* c) { return c ? c->adapt_passes_skipped : -1; }
long long promp_constraint_hvp_cached_passes(promp_ctx* c) { return c ? c->chvp_cached_passes : -1; }
long long promp_state_version(promp_ctx* c) { return c ? (long long)c->version_counter : -1; }
int promp_set_primal_cache(promp_ctx* c, int on) {
    NEED_CTX(c);
    c->primal_cache = on < 0 ? -1 : on != 0;
    return 0;
}
int promp_set_learn_std(promp_ctx* c, int on) {
    NEED_CTX(c);
    if (on && !c->learn_std) return fail(-3, "learn_std cannot be switched back on: the log_std step sizes were zeroed (set the step sizes again)");
    c->learn_std = on != 0;
    c->sizes_version = ++c->version_counter;
    return mask_log_std_step_sizes(c);
}
static int tasks_materialize(promp_ctx* c);
int promp_set_task_thetas(promp_ctx* c, const float* t) {
    NEED_CTX(c);
    c->tasks_shared = false;
    return params_in(c, c->theta_tasks, t, (size_t)c->d.n_tasks);
}
int promp_get_task_thetas(promp_ctx* c, float* t) {
    NEED_CTX(c);
    if (tasks_materialize(c)) return -2;
    return params_out(c, t, c->theta_tasks, (size_t)c->d.n_tasks);
}

int promp_set_adam_state(promp_ctx* c, const float* m, const float* v, int64_t t) {
    NEED_CTX(c);
    if (params_in(c, c->adam_m, m, 1) || params_in(c, c->adam_v, v, 1)) return -2;
    c->adam_t = t;
    return 0;
}
int promp_get_adam_state(promp_ctx* c, float* m, float* v, int64_t* t) {
    NEED_CTX(c);
    if (m && params_out(c, m, c->adam_m, 1)) return -2;
    if (v && params_out(c, v, c->adam_v, 1)) return -2;
    if (t) *t = c->adam_t;
    return 0;
}

// MetaPolicy.switch_to_pre_update (policies/base.py:173-179): every task's parameters are the meta-parameters again.  Nothing is
// launched here: the inner step reads theta with a task stride of zero, and the per-task copies are only written
// (tasks_materialize) for the entry points that hand them out or index them per task.
int promp_switch_to_pre_update(promp_ctx* c) {
    NEED_CTX(c);
    c->tasks_shared = true;
    return 0;
}
static int tasks_materialize(promp_ctx* c) {
    if (!c->tasks_shared) return 0;
    PROMP_LAUNCH(k_replicate, dim3((c->NP + 255) / 256), 256, 0, c->stream, c->theta_tasks, (const float*)c->theta, c->NP, c->d.n_tasks);
    HIPCHECK(hipGetLastError());
    c->tasks_shared = false;
    return 0;
}

int promp_inner_adapt(promp_ctx* c, int step, int inner_kind) {
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/true);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    // pre-update mode: all tasks start from theta itself (stride 0); the step writes every task's row of theta_tasks
    const float* cur = c->tasks_shared ? c->theta : c->theta_tasks;
    const long long st = c->tasks_shared ? 0 : c->NP;
    // From the meta-parameters on step 0 this IS the first inner pass of the meta-objective (pro_mp.py:113-128 rebuilds what
    // base.py:217-242 just ran): leave theta', the scalars and the primal cache where the first epoch looks for them.  The two
    // differ only in log_std entries below log(min_std) (raw here, gaussian_mlp_policy.py:182; clipped there, :71,163), which
    // enqueue_meta checks before it trusts the result.
    const bool leave = c->reuse_adapt && c->tasks_shared && step == 0 &&
                       (inner_kind == PROMP_INNER_RATIO || inner_kind == PROMP_INNER_LOGLIK);
    if (step == 0) c->adapt0.valid = false;       // (inner steps on later sampling steps touch nothing the record stands for)
    PassReq q;
    q.theta = cur; q.theta_stride = st; q.loss_kind = loss_kind_inner(inner_kind);
    q.red_mode = RED_STEP; q.cur = cur; q.cur_stride = st; q.next = c->theta_tasks;
    const bool cached = leave && primal_cache_on(c);
    if (cached && ensure_primal_cache(c, pass_slab(S))) return -2;
    q.cache = cached ? 1 : 0;
    if (leave) {
        q.next2 = c->chain + (size_t)c->d.n_tasks * c->NP;
        q.scal2 = c->scal_inner;
        q.ginner = c->train_sizes ? c->ginner.p : nullptr;     // ... and the gradient itself, the step sizes' first factor
    }
    c->tasks_shared = false;
    const int rc = launch_pass(c, pass_slab(S), q);
    if (rc) return rc;
    if (leave) {
        c->adapt0.valid = true; c->adapt0.theta_version = c->theta_version; c->adapt0.data_version = S.data_version;
        c->adapt0.sizes_version = c->sizes_version; c->adapt0.inner_kind = inner_kind; c->adapt0.cached = cached;
        c->adapt0.min_log_std = c->min_log_std; c->adapt0.learn_std = c->learn_std;
    }
    return 0;
}

int promp_policy_forward(promp_ctx* c, const float* obs, int batch, float* mean_out) {
    if (!c || !obs || !mean_out) return fail(-1, "NULL argument");
    if (batch < 1) return fail(-1, "batch must be positive");
    const int M = c->d.n_tasks, O = c->d.obs_dim, A = c->d.act_dim;
    const size_t n_obs = (size_t)M * batch * O, n_out = (size_t)M * batch * A;
    const size_t n_scr = c->family == PassFamily::Layered ? (size_t)M * batch * 2 * c->g_maxw : 0;
    if (c->fwd_buf.reserve(n_obs + n_out + n_scr, 2)) return -2;
    float* d_obs = c->fwd_buf;
    float* d_out = c->fwd_buf + n_obs;
    HIPCHECK(hipMemcpyAsync(d_obs, obs, sizeof(float) * n_obs, hipMemcpyHostToDevice, c->stream));
    ForwardArgs f;
    if (tasks_materialize(c)) return -2;
    f.obs = d_obs; f.theta_tasks = c->theta_tasks; f.mean = d_out;
    f.B = batch; f.O = O; f.A = A; f.H1 = c->d.hidden1; f.H2 = c->d.hidden2;
    if (c->family == PassFamily::Layered) {
        GenForwardArgs gf;
        gf.obs = d_obs; gf.theta_tasks = c->theta_tasks; gf.mean = d_out; gf.scratch = d_out + n_out;
        gf.B = batch; gf.NP = c->NP; gf.maxw = c->g_maxw; gf.act_kind = gen_act_kinds(&c->d);
        copy_layers(gf, c);
        PROMP_LAUNCH(k_gen_policy_forward, dim3(M), 256, 0, c->stream, gf);
    } else
    PROMP_LAUNCH(k_policy_forward, dim3(M), 256, 0, c->stream, f);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(mean_out, d_out, sizeof(float) * n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// fixed-length layout of a device-side rollout: path p of task i is rows [(i B + p) T, (i B + p + 1) T)
// (sc: the caller's scope, checked but not yet open)
static int begin_fixed_rollout(StepScope& sc, int B, int T) {
    if (sc.rc) return sc.rc;
    promp_ctx* c = sc.c;
    if (B < 1 || T < 1) return fail(-1, "envs_per_task and path_length must be positive");
    const int M = c->d.n_tasks;
    const long long rows = (long long)M * B * T;
    if (rows > c->d.max_rows) return fail(-1, "rollout of %lld rows exceeds max_rows = %d", rows, c->d.max_rows);
    std::vector<int32_t> tpo(M + 1), pro((size_t)M * B + 1);
    for (int i = 0; i <= M; ++i) tpo[i] = i * B;
    for (int p = 0; p <= M * B; ++p) pro[p] = p * T;
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    StepData& S = sc.S();
    clear_selection(c, sc.step);
    if (set_step_layout(c, S, c->stream, false, M * B, tpo.data(), pro.data())) return -2;
    S.has_policy = true;
    S.ls_per_row = 0;
    S.rollout_B = B; S.rollout_T = T;
    S.dev_policy_done = S.dev_filed = 0;
    return 0;
}

int promp_rollout_point_env(promp_ctx* c, int step, int envs_per_task, int path_length, const double* goals,
                            const double* start, const float* noise, const promp_point_env_opts* o) {
    if (!c || !goals || !start || !o) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (c->d.obs_dim != 2 || c->d.act_dim != 2) return fail(-1, "the point environment has obs_dim = act_dim = 2 (context: %d, %d)", c->d.obs_dim, c->d.act_dim);
    if (o->reward_type < 0 || o->reward_type > 2) return fail(-1, "unknown reward type %d", o->reward_type);
    if (begin_fixed_rollout(sc, envs_per_task, path_length)) return -2;
    const int M = c->d.n_tasks, B = envs_per_task, T = path_length;
    const long long rows = (long long)M * B * T;
    StepData& S = sc.S();
    S.data_version = ++c->version_counter;       // (the rollout's own bump behind the layout's: promp_state_version counts both)
    const size_t need = sizeof(double) * ((size_t)M * 2 + (size_t)M * B * 2) + sizeof(float) * (size_t)rows * 2;
    if (c->rollout_buf.reserve(need, 2)) return -2;
    double* d_goals = (double*)c->rollout_buf.p;
    double* d_start = d_goals + (size_t)M * 2;
    float* d_noise = (float*)(d_start + (size_t)M * B * 2);
    hipStream_t st = c->stream;
    HIPCHECK(hipMemcpyAsync(d_goals, goals, sizeof(double) * M * 2, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_start, start, sizeof(double) * M * B * 2, hipMemcpyHostToDevice, st));
    if (noise) HIPCHECK(hipMemcpyAsync(d_noise, noise, sizeof(float) * rows * 2, hipMemcpyHostToDevice, st));
    PointRolloutArgs a;
    if (tasks_materialize(c)) return -2;
    a.theta_tasks = c->theta_tasks; a.NP = c->NP; a.H1 = c->d.hidden1; a.H2 = c->d.hidden2;
    a.B = B; a.T = T; a.goals = d_goals; a.start = d_start; a.noise = noise ? d_noise : nullptr;
    a.seed = o->seed; a.stream = (unsigned)step;
    a.obs = S.obs; a.act = S.act; a.rew = S.rew; a.mean = S.old_mean; a.old_ls = S.old_ls;
    a.clip_infos = o->clip_infos; a.min_log_std = c->min_log_std;
    a.normalization_scale = o->normalization_scale; a.max_step = o->max_step; a.reward_type = o->reward_type; a.sparse_radius = o->sparse_radius;
    if (c->family == PassFamily::Layered) {          // any layer table: one workgroup per environment (promp_kernels_generic.h)
        GenPointRolloutArgs g;
        g.p = a; g.act_kind = gen_act_kinds(&c->d);
        copy_layers(g, c);
        PROMP_LAUNCH(k_gen_point_rollout, dim3(B, M), 256, gen_rollout_smem(2), st, g);
    } else
    PROMP_LAUNCH(k_point_rollout, dim3(M), 64, 0, st, a);
    HIPCHECK(hipGetLastError());
    S.ps.obs_range_valid = false;
    return 0;
}

// the box of a device-side start draw: lo <= hi and finite in every coordinate the environment has -> the kernels' form
static int point_start_box(const promp_point_start_opts* so, int state_dim, PointStartBox* bx) {
    *bx = PointStartBox{};
    for (int k = 0; k < state_dim; ++k) {
        if (!std::isfinite(so->lo[k]) || !std::isfinite(so->hi[k]))
            return fail(-1, "start bounds of coordinate %d are not finite: lo = %g, hi = %g", k, so->lo[k], so->hi[k]);
        if (so->lo[k] > so->hi[k]) return fail(-1, "start bounds of coordinate %d: lo = %g > hi = %g", k, so->lo[k], so->hi[k]);
        bx->lo[k] = so->lo[k];
        bx->hi[k] = so->hi[k];
    }
    bx->seed = so->seed;
    return 0;
}

int promp_draw_point_starts(promp_ctx* c, int step, int n_rows, int n_envs, int state_dim, const promp_point_start_opts* so, double* out) {
    if (!c || !so || !out) return fail(-1, "NULL argument");
    if (step < 0 || step > c->d.num_inner_steps) return fail(-1, "step %d out of range", step);
    if (n_rows < 1 || n_envs < 1) return fail(-1, "n_rows = %d and n_envs = %d must be positive", n_rows, n_envs);
    if (state_dim != 2 && state_dim != 4) return fail(-1, "state_dim = %d must be 2 or 4", state_dim);
    PointStartsArgs a;
    if (point_start_box(so, state_dim, &a.bx)) return -2;
    a.n = (long long)n_rows * n_envs;
    if (a.n > 0x7FFFFFFFll / 4) return fail(-1, "n_rows * n_envs = %lld start states are too many", a.n);
    const size_t n = (size_t)a.n * state_dim;
    if (c->rollout_buf.reserve(sizeof(double) * n, 2)) return -2;
    a.stream = (unsigned)step; a.state_dim = state_dim; a.out = (double*)c->rollout_buf.p;
    PROMP_LAUNCH(k_point_starts, dim3((unsigned)((a.n + 255) / 256)), 256, 0, c->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out, a.out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// start: the table [n_tasks][envs_per_task][state_dim], or NULL: drawn on the device from so (nothing but the task parameters and
// host noise is uploaded)
static int rollout_point_family(promp_ctx* c, int step, int envs_per_task, int path_length, const double* task_params,
                                const double* start, const promp_point_start_opts* so, const float* noise,
                                const promp_point_family_opts* o) {
    if (!c || !task_params || (!start && !so) || !o) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (o->kind < POINT_KIND_CORNER || o->kind > POINT_KIND_MOMENTUM) return fail(-1, "unknown environment kind %d", o->kind);
    const int task_dim = o->kind == POINT_KIND_WALLS ? 6 : 2, state_dim = o->kind == POINT_KIND_MOMENTUM ? 4 : 2;
    if (o->task_dim != task_dim) return fail(-1, "task_dim = %d, environment kind %d has task_dim = %d", o->task_dim, o->kind, task_dim);
    if (c->d.obs_dim != state_dim) return fail(-1, "environment kind %d has obs_dim = %d (context: %d)", o->kind, state_dim, c->d.obs_dim);
    if (c->d.act_dim != 2) return fail(-1, "the point environments have act_dim = 2 (context: %d)", c->d.act_dim);
    if (o->reward_type < 0 || o->reward_type > 2) return fail(-1, "unknown reward type %d", o->reward_type);
    PointStartBox bx = {};
    if (!start && point_start_box(so, state_dim, &bx)) return -2;
    if (begin_fixed_rollout(sc, envs_per_task, path_length)) return -2;
    const int M = c->d.n_tasks, B = envs_per_task, T = path_length;
    const long long rows = (long long)M * B * T;
    StepData& S = sc.S();
    S.data_version = ++c->version_counter;
    const size_t n_task = (size_t)M * task_dim, n_start = start ? (size_t)M * B * state_dim : 0;
    if (c->rollout_buf.reserve(sizeof(double) * (n_task + n_start) + sizeof(float) * (size_t)rows * 2, 2)) return -2;
    double* d_task = (double*)c->rollout_buf.p;
    double* d_start = d_task + n_task;
    float* d_noise = (float*)(d_start + n_start);
    hipStream_t st = c->stream;
    HIPCHECK(hipMemcpyAsync(d_task, task_params, sizeof(double) * n_task, hipMemcpyHostToDevice, st));
    if (start) HIPCHECK(hipMemcpyAsync(d_start, start, sizeof(double) * n_start, hipMemcpyHostToDevice, st));
    if (noise) HIPCHECK(hipMemcpyAsync(d_noise, noise, sizeof(float) * rows * 2, hipMemcpyHostToDevice, st));
    PointFamilyArgs f;
    PointRolloutArgs& a = f.p;
    if (tasks_materialize(c)) return -2;
    a.theta_tasks = c->theta_tasks; a.NP = c->NP; a.H1 = c->d.hidden1; a.H2 = c->d.hidden2;
    a.B = B; a.T = T; a.goals = d_task; a.start = start ? d_start : nullptr; a.noise = noise ? d_noise : nullptr;
    a.seed = o->seed; a.stream = (unsigned)step;
    a.obs = S.obs; a.act = S.act; a.rew = S.rew; a.mean = S.old_mean; a.old_ls = S.old_ls;
    a.clip_infos = o->clip_infos; a.min_log_std = c->min_log_std;
    a.normalization_scale = o->normalization_scale; a.max_step = o->max_step; a.reward_type = o->reward_type; a.sparse_radius = o->sparse_radius;
    f.kind = o->kind; f.task_dim = task_dim; f.state_dim = state_dim;
    if (c->family == PassFamily::Layered) {
        GenPointFamilyArgs g;
        g.f = f; g.act_kind = gen_act_kinds(&c->d);
        copy_layers(g, c);
        if (start) PROMP_LAUNCH(k_gen_point_family_rollout<false>, dim3(B, M), 256, gen_rollout_smem(state_dim), st, g, bx);
        else PROMP_LAUNCH(k_gen_point_family_rollout<true>, dim3(B, M), 256, gen_rollout_smem(state_dim), st, g, bx);
    } else if (start)
    PROMP_LAUNCH(k_point_family_rollout<false>, dim3(M), 64, 0, st, f, bx);
    else
    PROMP_LAUNCH(k_point_family_rollout<true>, dim3(M), 64, 0, st, f, bx);
    HIPCHECK(hipGetLastError());
    S.ps.obs_range_valid = false;
    return 0;
}

int promp_rollout_point_family(promp_ctx* c, int step, int envs_per_task, int path_length, const double* task_params,
                               const double* start, const float* noise, const promp_point_family_opts* o) {
    if (!start) return fail(-1, "NULL argument");
    return rollout_point_family(c, step, envs_per_task, path_length, task_params, start, nullptr, noise, o);
}

int promp_rollout_point_family_dev(promp_ctx* c, int step, int envs_per_task, int path_length, const double* task_params,
                                   const promp_point_start_opts* starts, const float* noise, const promp_point_family_opts* o) {
    if (!starts) return fail(-1, "promp_rollout_point_family_dev: starts is NULL");
    return rollout_point_family(c, step, envs_per_task, path_length, task_params, nullptr, starts, noise, o);
}

int promp_begin_rollout(promp_ctx* c, int step, int envs_per_task, int path_length) {
    NEED_CTX(c);
    StepScope sc(c, step);
    if (begin_fixed_rollout(sc, envs_per_task, path_length)) return -2;
    sc.S().rollout_ragged = false;
    return 0;
}

int promp_begin_collection(promp_ctx* c, int step, int envs_per_task, int max_steps) {
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (envs_per_task < 1 || max_steps < 1) return fail(-1, "envs_per_task and max_steps must be positive");
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    StepData& S = sc.S();
    const size_t need = (size_t)max_steps * c->d.n_tasks * envs_per_task * (c->d.obs_dim + 2 * c->d.act_dim);
    if (c->stage_rows.reserve(need, 1)) return -2;
    S.rollout_B = envs_per_task; S.rollout_T = max_steps; S.rollout_ragged = true;
    S.dev_policy_done = S.dev_filed = 0;
    S.has_policy = false; S.processed = false; S.has_adv = false;
    return 0;
}

// The tail of a ragged collection, shared by promp_end_collection (tables from the host: h_env / h_start, rewards h_rewards in path
// order) and promp_collect_point_family (tables already on the device: d_env / d_start, rewards gathered from the staged d_rew):
// the layout, the finished episodes copied from the staging rows into the slab, the step's flags.  sc is open.
static int finish_collection(StepScope& sc, int n_paths, const int32_t* tpo, const int32_t* pro, const int32_t* h_env, const int32_t* h_start,
                             const int32_t* d_env, const int32_t* d_start, const float* h_rewards, const float* d_rew) {
    promp_ctx* c = sc.c;
    StepData& S = sc.S();
    const int M = c->d.n_tasks, B = S.rollout_B, O = c->d.obs_dim, A = c->d.act_dim;
    clear_selection(c, sc.step);
    if (set_step_layout(c, S, c->stream, false, n_paths, tpo, pro)) return -2;
    // the finished episodes: staging rows -> slab rows in path order
    if (h_env) {
        if (c->rollout_buf.reserve(sizeof(int32_t) * 2 * (size_t)n_paths, 2)) return -2;
        int32_t* up_env = (int32_t*)c->rollout_buf.p;
        int32_t* up_start = up_env + n_paths;
        HIPCHECK(hipMemcpyAsync(up_env, h_env, sizeof(int32_t) * n_paths, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(up_start, h_start, sizeof(int32_t) * n_paths, hipMemcpyHostToDevice, c->stream));
        d_env = up_env; d_start = up_start;
    }
    GatherPathsArgs g;
    const size_t n_rows = (size_t)S.rollout_T * M * B;
    g.obs_in = c->stage_rows; g.act_in = c->stage_rows + n_rows * O; g.mean_in = g.act_in + n_rows * A;
    g.obs = S.obs; g.act = S.act; g.mean = S.old_mean;
    g.path_env = d_env; g.path_start = d_start; g.path_row_offsets = S.path_row_offsets;
    g.n_envs = M * B; g.O = O; g.A = A;
    g.rew_in = d_rew; g.rew = S.rew;
    PROMP_LAUNCH(k_gather_paths, dim3(n_paths), 256, 0, c->stream, g);
    HIPCHECK(hipGetLastError());
    if (h_rewards) HIPCHECK(hipMemcpyAsync(S.rew, h_rewards, sizeof(float) * pro[n_paths], hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    S.has_policy = true; S.ls_per_row = 0; S.has_rew64 = false; S.processed = false; S.has_adv = false;
    S.rollout_ragged = false; S.rollout_B = 0;
    S.ps.obs_range_valid = false;
    return 0;
}

int promp_end_collection(promp_ctx* c, int step, int n_paths, const int32_t* task_path_offsets, const int32_t* path_env,
                         const int32_t* path_start, const int32_t* path_len, const float* rewards) {
    if (!c || !task_path_offsets || !path_env || !path_start || !path_len || !rewards) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (!S.rollout_ragged || S.rollout_B < 1) return fail(-3, "promp_begin_collection has not been called for step %d", step);
    const int M = c->d.n_tasks, B = S.rollout_B;
    if (n_paths < 1 || n_paths > c->d.max_paths) return fail(-1, "%d paths outside [1, max_paths = %d]", n_paths, c->d.max_paths);
    std::vector<int32_t> pro((size_t)n_paths + 1, 0);
    for (int p = 0; p < n_paths; ++p) {
        if (path_len[p] < 1 || path_start[p] < 0 || path_start[p] + path_len[p] > S.rollout_T || path_env[p] < 0 || path_env[p] >= M * B)
            return fail(-1, "path %d (environment %d, steps [%d, %d)) lies outside the collection", p, path_env[p], path_start[p], path_start[p] + path_len[p]);
        pro[p + 1] = pro[p] + path_len[p];
    }
    if (pro[n_paths] > c->d.max_rows) return fail(-1, "%d collected rows exceed max_rows = %d", pro[n_paths], c->d.max_rows);
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    return finish_collection(sc, n_paths, task_path_offsets, pro.data(), path_env, path_start, nullptr, nullptr, rewards, nullptr);
}

// Whole collection on the device: k_point_collect, k_collect_stop, k_collect_tables (promp_kernels_rollout.h); only the tables come
// back.  Every refusal leaves the step without a layout of this call: the slab is touched by finish_collection alone.
// nm: the normalize wrapper's options, or NULL / both flags 0: the plain collection.  With a flag set the start table has
// max_steps + 1 rows and the context's running moments (promp_point_norm_set) advance to their state after the stop step.
// start: the table, or NULL: every reset() drawn on the device from so -- no table is reserved or uploaded.
static int collect_point_family(promp_ctx* c, int step, int envs_per_task, const double* task_params, const double* start,
                                const promp_point_start_opts* so,
                                const float* noise, const promp_point_collect_opts* o, const promp_point_norm_opts* nm,
                                int32_t* n_paths_out, int32_t* n_steps_out,
                                int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len) {
    if (!c || !task_params || (!start && !so) || !o || !n_paths_out || !n_steps_out || !task_path_offsets || !path_env || !path_start || !path_len)
        return fail(-1, "NULL argument");
    const bool norm = nm && (nm->normalize_obs || nm->normalize_reward);
    if (nm) {
        if (!(nm->obs_alpha >= 0.0 && nm->obs_alpha <= 1.0)) return fail(-1, "obs_alpha = %g outside [0, 1]", nm->obs_alpha);
        if (!(nm->reward_alpha >= 0.0 && nm->reward_alpha <= 1.0)) return fail(-1, "reward_alpha = %g outside [0, 1]", nm->reward_alpha);
    }
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    const promp_point_family_opts& e = o->env;
    if (e.kind < POINT_KIND_CORNER || e.kind > POINT_KIND_GOAL) return fail(-1, "unknown environment kind %d", e.kind);
    const int task_dim = e.kind == POINT_KIND_WALLS ? 6 : 2, state_dim = e.kind == POINT_KIND_MOMENTUM ? 4 : 2;
    if (e.task_dim != task_dim) return fail(-1, "task_dim = %d, environment kind %d has task_dim = %d", e.task_dim, e.kind, task_dim);
    if (c->d.obs_dim != state_dim) return fail(-1, "environment kind %d has obs_dim = %d (context: %d)", e.kind, state_dim, c->d.obs_dim);
    if (c->d.act_dim != 2) return fail(-1, "the point environments have act_dim = 2 (context: %d)", c->d.act_dim);
    if (e.reward_type < 0 || e.reward_type > 2) return fail(-1, "unknown reward type %d", e.reward_type);
    if (o->max_path_length < 1) return fail(-1, "max_path_length = %d must be positive", o->max_path_length);
    if (envs_per_task < 1 || o->max_steps < 1) return fail(-1, "envs_per_task and max_steps must be positive");
    if (o->total_samples < 1) return fail(-1, "total_samples must be positive");
    PointStartBox bx = {};
    if (!start && point_start_box(so, state_dim, &bx)) return -2;
    const int M = c->d.n_tasks, B = envs_per_task, O = state_dim, A = 2, S_max = o->max_steps, max_paths = c->d.max_paths;
    const long long n_envs = (long long)M * B, stage = n_envs * S_max;
    if (stage > 0x7FFFFFFFll / 4) return fail(-1, "max_steps * environments = %lld staging rows are too many", stage);
    const int W = 2 * O + 2;                                       // moments per environment
    if (norm) {
        if (c->point_norm_envs == 0) return fail(-3, "a normalisation flag is set but promp_point_norm_set has not been called");
        if (c->point_norm_envs != n_envs || c->point_norm_dim != O)
            return fail(-1, "the normalisation state was set for %d environments of state_dim %d, the collection has %lld of %d",
                        c->point_norm_envs, c->point_norm_dim, n_envs, O);
    }
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    StepData& S = sc.S();
    if (c->stage_rows.reserve((size_t)stage * (O + 2 * A), 1)) return -2;
    if (norm && c->point_norm_stage.reserve((size_t)stage * W, 1)) return -2;
    S.has_policy = false; S.processed = false; S.has_adv = false;
    // one block: doubles (task parameters, start table), the stop record, floats (noise, staged rewards), then the integer tables
    const size_t n_task = (size_t)M * task_dim, n_start = start ? (size_t)(stage + (norm ? n_envs : 0)) * O : 0;
    const size_t n_noise = noise ? (size_t)stage * 2 : 0;
    const size_t n_int = (size_t)stage + S_max + M + (M + 1) + 3 * (size_t)max_paths;
    if (c->rollout_buf.reserve(sizeof(double) * (n_task + n_start) + sizeof(long long) * 4 + sizeof(float) * (n_noise + (size_t)stage) +
                               sizeof(int32_t) * n_int, 2)) return -2;
    double* d_task = (double*)c->rollout_buf.p;
    double* d_start = d_task + n_task;
    long long* d_stop = (long long*)(d_start + n_start);
    float* d_noise = (float*)(d_stop + 4);
    float* d_rew = d_noise + n_noise;
    int32_t* d_end = (int32_t*)(d_rew + stage);
    int32_t* d_sum = d_end + stage;
    int32_t* d_count = d_sum + S_max;
    int32_t* d_tpo = d_count + M;
    int32_t* d_env = d_tpo + (M + 1);
    int32_t* d_pstart = d_env + max_paths;
    int32_t* d_len = d_pstart + max_paths;
    hipStream_t st = c->stream;
    HIPCHECK(hipMemcpyAsync(d_task, task_params, sizeof(double) * n_task, hipMemcpyHostToDevice, st));
    if (start) HIPCHECK(hipMemcpyAsync(d_start, start, sizeof(double) * n_start, hipMemcpyHostToDevice, st));
    if (noise) HIPCHECK(hipMemcpyAsync(d_noise, noise, sizeof(float) * n_noise, hipMemcpyHostToDevice, st));
    if (tasks_materialize(c)) return -2;
    PointCollectArgs k;
    PointRolloutArgs& a = k.f.p;
    a.theta_tasks = c->theta_tasks; a.NP = c->NP; a.H1 = c->d.hidden1; a.H2 = c->d.hidden2;
    a.B = B; a.T = S_max; a.goals = d_task; a.start = start ? d_start : nullptr; a.noise = noise ? d_noise : nullptr;
    a.seed = e.seed; a.stream = (unsigned)step;
    a.obs = c->stage_rows; a.act = c->stage_rows + (size_t)stage * O; a.mean = a.act + (size_t)stage * A; a.rew = nullptr;
    a.old_ls = S.old_ls;
    a.clip_infos = e.clip_infos; a.min_log_std = c->min_log_std;
    a.normalization_scale = e.normalization_scale; a.max_step = e.max_step; a.reward_type = e.reward_type; a.sparse_radius = e.sparse_radius;
    k.f.kind = e.kind; k.f.task_dim = task_dim; k.f.state_dim = state_dim;
    k.rew_stage = d_rew; k.end_len = d_end;
    k.max_steps = S_max; k.max_path_length = o->max_path_length; k.n_envs = (int)n_envs; k.done_radius = o->done_radius;
    PointNormArgs pn = {};
    if (norm) {
        pn.normalize_obs = nm->normalize_obs != 0; pn.normalize_reward = nm->normalize_reward != 0;
        pn.obs_alpha = nm->obs_alpha; pn.reward_alpha = nm->reward_alpha;
        pn.moments = c->point_norm; pn.stage = c->point_norm_stage;
    }
    if (c->family == PassFamily::Layered) {
        GenPointCollectArgs g;
        g.c = k; g.act_kind = gen_act_kinds(&c->d);
        copy_layers(g, c);
        if (norm) {
            GenPointNormCollectArgs gn;
            gn.g = g; gn.n = pn;
            if (start) PROMP_LAUNCH(k_gen_point_norm_collect<false>, dim3(B, M), 256, gen_rollout_smem(state_dim), st, gn, bx);
            else PROMP_LAUNCH(k_gen_point_norm_collect<true>, dim3(B, M), 256, gen_rollout_smem(state_dim), st, gn, bx);
        } else if (start)
        PROMP_LAUNCH(k_gen_point_collect<false>, dim3(B, M), 256, gen_rollout_smem(state_dim), st, g, bx);
        else
        PROMP_LAUNCH(k_gen_point_collect<true>, dim3(B, M), 256, gen_rollout_smem(state_dim), st, g, bx);
    } else if (norm) {
        PointNormCollectArgs kn;
        kn.c = k; kn.n = pn;
        if (start) PROMP_LAUNCH(k_point_norm_collect<false>, dim3(M), 64, 0, st, kn, bx);
        else PROMP_LAUNCH(k_point_norm_collect<true>, dim3(M), 64, 0, st, kn, bx);
    } else if (start)
    PROMP_LAUNCH(k_point_collect<false>, dim3(M), 64, 0, st, k, bx);
    else
    PROMP_LAUNCH(k_point_collect<true>, dim3(M), 64, 0, st, k, bx);
    HIPCHECK(hipGetLastError());
    CollectStopArgs cs;
    cs.end_len = d_end; cs.step_sum = d_sum; cs.out = d_stop; cs.max_steps = S_max; cs.n_envs = (int)n_envs; cs.total_samples = o->total_samples;
    PROMP_LAUNCH(k_collect_stop, dim3(1), 256, 0, st, cs);
    CollectTablesArgs ct;
    ct.end_len = d_end; ct.stop = d_stop; ct.task_count = d_count; ct.task_path_offsets = d_tpo;
    ct.path_env = d_env; ct.path_start = d_pstart; ct.path_len = d_len;
    ct.B = B; ct.max_steps = S_max; ct.n_envs = (int)n_envs; ct.n_tasks = M; ct.max_paths = max_paths; ct.write = 0;
    PROMP_LAUNCH(k_collect_tables, dim3(M), 64, 0, st, ct);
    PROMP_LAUNCH(k_collect_offsets, dim3(1), 64, 0, st, (const int*)d_count, d_tpo, M);
    ct.write = 1;
    PROMP_LAUNCH(k_collect_tables, dim3(M), 64, 0, st, ct);
    HIPCHECK(hipGetLastError());
    long long stop[3] = {-1, 0, 1};
    std::vector<int32_t> tpo((size_t)M + 1, 0);
    HIPCHECK(hipMemcpyAsync(stop, d_stop, sizeof stop, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(tpo.data(), d_tpo, sizeof(int32_t) * (M + 1), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (stop[2] != 0 || stop[0] < 0)
        return fail(-1, "max_steps = %d vectorised steps do not reach total_samples = %lld", S_max, (long long)o->total_samples);
    if (stop[1] > c->d.max_rows) return fail(-1, "%lld collected rows exceed max_rows = %d", stop[1], c->d.max_rows);
    const int n_paths = tpo[M];
    if (n_paths < 1 || n_paths > max_paths) return fail(-1, "%d paths outside [1, max_paths = %d]", n_paths, max_paths);
    std::string empty;
    for (int i = 0; i < M; ++i)
        if (tpo[i + 1] == tpo[i]) empty += (empty.empty() ? "" : ", ") + std::to_string(i);
    if (!empty.empty())
        return fail(-1, "no finished episode for task(s) [%s] within total_samples = %lld (envs_per_task = %d, max_path_length = %d)",
                    empty.c_str(), (long long)o->total_samples, B, o->max_path_length);
    HIPCHECK(hipMemcpyAsync(path_env, d_env, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(path_start, d_pstart, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(path_len, d_len, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    std::vector<int32_t> pro((size_t)n_paths + 1, 0);
    for (int p = 0; p < n_paths; ++p) {
        if (path_len[p] < 1 || path_start[p] < 0 || path_start[p] + path_len[p] > S_max || path_env[p] < 0 || path_env[p] >= n_envs)
            return fail(-2, "path %d (environment %d, steps [%d, %d)) lies outside the collection", p, path_env[p], path_start[p], path_start[p] + path_len[p]);
        pro[p + 1] = pro[p] + path_len[p];
    }
    if (pro[n_paths] != stop[1]) return fail(-2, "the path tables hold %d rows, the stop record %lld", pro[n_paths], stop[1]);
    S.rollout_B = B; S.rollout_T = S_max; S.rollout_ragged = true;       // (what finish_collection reads, and clears)
    if (finish_collection(sc, n_paths, tpo.data(), pro.data(), nullptr, nullptr, d_env, d_pstart, nullptr, d_rew)) return -2;
    if (norm) {                        // accepted and installed: the wrapper state after the stop step becomes the context's
        PointNormCommitArgs pc;
        pc.stage = c->point_norm_stage; pc.stop = d_stop; pc.moments = c->point_norm; pc.W = W; pc.n_envs = (int)n_envs; pc.max_steps = S_max;
        PROMP_LAUNCH(k_point_norm_commit, dim3((unsigned)((n_envs + 255) / 256)), 256, 0, st, pc);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(st));
    }
    for (int i = 0; i <= M; ++i) task_path_offsets[i] = tpo[i];
    *n_paths_out = n_paths;
    *n_steps_out = (int32_t)stop[0] + 1;
    return 0;
}

int promp_collect_point_family(promp_ctx* c, int step, int envs_per_task, const double* task_params, const double* start,
                               const float* noise, const promp_point_collect_opts* o, int32_t* n_paths_out, int32_t* n_steps_out,
                               int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len) {
    if (!start) return fail(-1, "NULL argument");
    return collect_point_family(c, step, envs_per_task, task_params, start, nullptr, noise, o, nullptr, n_paths_out, n_steps_out,
                                task_path_offsets, path_env, path_start, path_len);
}

int promp_collect_point_family_norm(promp_ctx* c, int step, int envs_per_task, const double* task_params, const double* start,
                                    const float* noise, const promp_point_collect_opts* o, const promp_point_norm_opts* norm,
                                    int32_t* n_paths_out, int32_t* n_steps_out, int32_t* task_path_offsets, int32_t* path_env,
                                    int32_t* path_start, int32_t* path_len) {
    if (!norm || !start) return fail(-1, "NULL argument");
    return collect_point_family(c, step, envs_per_task, task_params, start, nullptr, noise, o, norm, n_paths_out, n_steps_out,
                                task_path_offsets, path_env, path_start, path_len);
}

int promp_collect_point_family_dev(promp_ctx* c, int step, int envs_per_task, const double* task_params,
                                   const promp_point_start_opts* starts, const float* noise, const promp_point_collect_opts* o,
                                   const promp_point_norm_opts* norm, int32_t* n_paths_out, int32_t* n_steps_out,
                                   int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len) {
    if (!starts) return fail(-1, "promp_collect_point_family_dev: starts is NULL");
    return collect_point_family(c, step, envs_per_task, task_params, nullptr, starts, noise, o, norm, n_paths_out, n_steps_out,
                                task_path_offsets, path_env, path_start, path_len);
}

int promp_point_norm_set(promp_ctx* c, int n_envs, int state_dim, const double* moments) {
    if (!c || !moments) return fail(-1, "NULL argument");
    if (n_envs < 1 || (state_dim != 2 && state_dim != 4)) return fail(-1, "n_envs = %d must be positive and state_dim = %d 2 or 4", n_envs, state_dim);
    const size_t n = (size_t)n_envs * (2 * state_dim + 2);
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (c->point_norm.reserve(n, 1)) return -2;
    HIPCHECK(hipMemcpyAsync(c->point_norm.p, moments, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    c->point_norm_envs = n_envs; c->point_norm_dim = state_dim;
    return 0;
}

int promp_point_norm_get(promp_ctx* c, int n_envs, int state_dim, double* moments) {
    if (!c || !moments) return fail(-1, "NULL argument");
    if (c->point_norm_envs == 0) return fail(-3, "promp_point_norm_set has not been called");
    if (c->point_norm_envs != n_envs || c->point_norm_dim != state_dim)
        return fail(-1, "the normalisation state was set for %d environments of state_dim %d, asked for %d of %d",
                    c->point_norm_envs, c->point_norm_dim, n_envs, state_dim);
    HIPCHECK(hipMemcpyAsync(moments, c->point_norm.p, sizeof(double) * (size_t)n_envs * (2 * state_dim + 2), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// One vectorised policy step of a rollout in progress: d_obs [n_tasks][B][O] and d_act [n_tasks][B][A] are device memory, the rows go
// to the slab (fixed horizon) or to the staging rows (ragged collection).  Shared by promp_policy_step and promp_policy_step_dev:
// the same kernel, rows, Philox counter and stream word whoever owns the two arrays.
static int launch_policy_step(promp_ctx* c, StepData& S, int step, int t, const float* d_obs, uint64_t seed, int clip_infos, float* d_act) {
    const int M = c->d.n_tasks, B = S.rollout_B, T = S.rollout_T, O = c->d.obs_dim, A = c->d.act_dim;
    hipStream_t st = c->stream;
    PolicyStepArgs a;
    if (tasks_materialize(c)) return -2;
    a.obs_in = d_obs; a.theta_tasks = c->theta_tasks;
    a.obs = S.obs; a.act = S.act; a.mean = S.old_mean; a.old_ls = S.old_ls; a.actions_out = d_act;
    a.row_env_stride = T; a.row_t_stride = 1;
    if (S.rollout_ragged) {       // (s, env) rows of the staging area
        const size_t n_rows = (size_t)T * M * B;
        a.obs = c->stage_rows; a.act = c->stage_rows + n_rows * O; a.mean = a.act + n_rows * A;
        a.row_env_stride = 1; a.row_t_stride = (long long)M * B;
    }
    a.B = B; a.T = T; a.t = t; a.O = O; a.A = A; a.H1 = c->d.hidden1; a.H2 = c->d.hidden2; a.NP = c->NP;
    a.clip_infos = clip_infos; a.min_log_std = c->min_log_std;
    a.seed = seed; a.stream = (unsigned)step;
    if (c->family == PassFamily::Layered) {          // any layer table: one workgroup per environment (promp_kernels_generic.h)
        GenPolicyStepArgs g;
        g.p = a; g.act_kind = gen_act_kinds(&c->d);
        copy_layers(g, c);
        PROMP_LAUNCH(k_gen_policy_step, dim3(B, M), 256, gen_rollout_smem(O), st, g);
    } else
    PROMP_LAUNCH(k_policy_step, dim3((B + 63) / 64, M), 64, 0, st, a);
    HIPCHECK(hipGetLastError());
    S.ps.obs_range_valid = false;
    return 0;
}

int promp_policy_step(promp_ctx* c, int step, int t, const float* obs, uint64_t seed, int clip_infos, float* actions_out) {
    if (!c || !obs || !actions_out) return fail(-1, "NULL argument");
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (S.rollout_B < 1) return fail(-3, "promp_begin_rollout has not been called for step %d", step);
    const int M = c->d.n_tasks, B = S.rollout_B, T = S.rollout_T, O = c->d.obs_dim, A = c->d.act_dim;
    if (t < 0 || t >= T) return fail(-1, "time step %d outside the horizon %d", t, T);
    const size_t n_obs = (size_t)M * B * O, n_act = (size_t)M * B * A;
    if (c->rollout_buf.reserve(sizeof(float) * (n_obs + n_act), 2)) return -2;
    float* d_obs = (float*)c->rollout_buf.p;
    float* d_act = d_obs + n_obs;
    hipStream_t st = c->stream;
    HIPCHECK(hipMemcpyAsync(d_obs, obs, sizeof(float) * n_obs, hipMemcpyHostToDevice, st));
    if (launch_policy_step(c, S, step, t, d_obs, seed, clip_infos, d_act)) return -2;
    HIPCHECK(hipMemcpyAsync(actions_out, d_act, sizeof(float) * n_act, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

int promp_set_rewards(promp_ctx* c, int step, const float* rew) {
    if (!c || !rew) return fail(-1, "NULL argument");
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/true);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    HIPCHECK(hipMemcpyAsync(S.rew, rew, sizeof(float) * S.n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    S.processed = false;
    S.has_rew64 = false;
    return 0;
}

int promp_set_rewards_f64(promp_ctx* c, int step, const double* rew) {
    if (!c || !rew) return fail(-1, "NULL argument");
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/true);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (!S.rew64 && S.rew64.alloc((size_t)c->d.max_rows)) return -2;
    std::vector<float> r32((size_t)S.n_rows);
    for (int i = 0; i < S.n_rows; ++i) r32[i] = (float)rew[i];
    HIPCHECK(hipMemcpyAsync(S.rew64, rew, sizeof(double) * S.n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(S.rew, r32.data(), sizeof(float) * S.n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    S.processed = false;
    S.has_rew64 = true;
    return 0;
}

// ---- environments that live on the device: the *_dev rollout entry points ----------------------------------------------------
}  // extern "C"
namespace {

// a caller pointer a kernel or a device-side copy is about to read or write through
int check_dev_ptr(const char* what, const void* p) {
    if (!p) return fail(-1, "%s is NULL", what);
    if (!promp_gpu_readable(p))
        return fail(-1, "%s = %p is neither device nor page-locked host memory: the GPU cannot read it", what, p);
    return 0;
}

// Ordering against the stream the caller's simulator enqueues on (0: the null stream).  enter: the context's stream waits for what
// the producer has enqueued so far (its observations, rewards, flags are complete before a kernel here reads them); leave: the
// producer waits for what the context has enqueued so far (it may overwrite its inputs and read the outputs in stream order).
// Two events per context, timing disabled, created with the first call; no stream is created.
int producer_enter(promp_ctx* c, void* producer_stream) {
    if (!c->ev_producer) HIPCHECK(hipEventCreateWithFlags(&c->ev_producer.h, hipEventDisableTiming));
    if (!c->ev_consumer) HIPCHECK(hipEventCreateWithFlags(&c->ev_consumer.h, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(c->ev_producer, (hipStream_t)producer_stream));
    HIPCHECK(hipStreamWaitEvent(c->stream, c->ev_producer, 0));
    return 0;
}
int producer_leave(promp_ctx* c, void* producer_stream) {
    HIPCHECK(hipEventRecord(c->ev_consumer, c->stream));
    HIPCHECK(hipStreamWaitEvent((hipStream_t)producer_stream, c->ev_consumer, 0));
    return 0;
}

// the integer block of a device-side collection (promp_ctx::dev_tables), for a staging area of max_steps * n_envs rows
struct DevCollectViews {
    int *end_len, *ep_len, *step_sum, *count, *tpo, *env, *start, *len;
    size_t n_int;
};
DevCollectViews dev_collect_views(const promp_ctx* c, int max_steps, long long n_envs) {
    const size_t stage = (size_t)max_steps * (size_t)n_envs, M = (size_t)c->d.n_tasks, P = (size_t)c->d.max_paths;
    DevCollectViews v;
    v.end_len = c->dev_tables.p;
    v.ep_len = v.end_len + stage;
    v.step_sum = v.ep_len + n_envs;
    v.count = v.step_sum + max_steps;
    v.tpo = v.count + M;
    v.env = v.tpo + (M + 1);
    v.start = v.env + P;
    v.len = v.start + P;
    v.n_int = stage + (size_t)n_envs + (size_t)max_steps + M + (M + 1) + 3 * P;
    return v;
}

// the checks promp_collection_progress and promp_end_collection_dev share; -> the open collection's step data
int dev_collection_of(StepScope& sc, const char* who, long long total_samples) {
    if (sc.rc) return sc.rc;
    const StepData& S = sc.S();
    if (!S.rollout_ragged || S.rollout_B < 1) return fail(-3, "%s: promp_begin_collection has not been called for step %d", who, sc.step);
    if (total_samples < 1) return fail(-1, "%s: total_samples must be positive", who);
    return 0;
}

// k_collect_stop over the steps filed so far -> stop[3] on the host (synchronises)
int dev_collect_stop(promp_ctx* c, const StepData& S, long long total_samples, long long* stop) {
    const long long n_envs = (long long)c->d.n_tasks * S.rollout_B;
    const DevCollectViews v = dev_collect_views(c, S.rollout_T, n_envs);
    CollectStopArgs cs;
    cs.end_len = v.end_len; cs.step_sum = v.step_sum; cs.out = c->dev_stop; cs.max_steps = S.dev_filed; cs.n_envs = (int)n_envs;
    cs.total_samples = total_samples;
    PROMP_LAUNCH(k_collect_stop, dim3(1), 256, 0, c->stream, cs);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(stop, c->dev_stop.p, sizeof(long long) * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace
extern "C" {

int promp_check_device_pointer(const void* p) { return check_dev_ptr("pointer", p) ? -1 : 0; }

void* promp_dev_alloc(promp_ctx* c, size_t bytes) {
    if (!c) {
        fail(-1, "ctx is NULL");
        return nullptr;
    }
    void* p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        fail(-2, "hipMalloc of %zu bytes failed", bytes);
        return nullptr;
    }
    return p;
}
void promp_dev_free(promp_ctx* c, void* p) {
    if (c && p) (void)hipFree(p);
}
int promp_dev_upload(promp_ctx* c, void* dst, const void* src, size_t bytes) {
    NEED_CTX(c);
    if (check_dev_ptr("promp_dev_upload: dst", dst)) return -1;
    if (!src) return fail(-1, "promp_dev_upload: src is NULL");
    HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
int promp_dev_download(promp_ctx* c, void* dst, const void* src, size_t bytes) {
    NEED_CTX(c);
    if (check_dev_ptr("promp_dev_download: src", src)) return -1;
    if (!dst) return fail(-1, "promp_dev_download: dst is NULL");
    HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int promp_policy_step_dev(promp_ctx* c, int step, int t, const float* d_obs, uint64_t seed, int clip_infos, float* d_actions,
                          void* producer_stream) {
    NEED_CTX(c);
    if (check_dev_ptr("promp_policy_step_dev: d_obs", d_obs) || check_dev_ptr("promp_policy_step_dev: d_actions", d_actions)) return -1;
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (S.rollout_B < 1) return fail(-3, "promp_begin_rollout has not been called for step %d", step);
    if (t < 0 || t >= S.rollout_T) return fail(-1, "time step %d outside the horizon %d", t, S.rollout_T);
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    if (producer_enter(c, producer_stream)) return -2;
    if (launch_policy_step(c, S, step, t, d_obs, seed, clip_infos, d_actions)) return -2;
    if (producer_leave(c, producer_stream)) return -2;
    S.dev_policy_done = std::max(S.dev_policy_done, t + 1);
    return 0;
}

int promp_file_step_dev(promp_ctx* c, int step, int s, const float* d_rewards, const uint8_t* d_done, int max_path_length,
                        uint8_t* d_ended_out, void* producer_stream) {
    NEED_CTX(c);
    if (check_dev_ptr("promp_file_step_dev: d_rewards", d_rewards)) return -1;
    if (d_done && check_dev_ptr("promp_file_step_dev: d_done", d_done)) return -1;
    if (d_ended_out && check_dev_ptr("promp_file_step_dev: d_ended_out", d_ended_out)) return -1;
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (S.rollout_B < 1) return fail(-3, "promp_begin_rollout / promp_begin_collection has not been called for step %d", step);
    const int M = c->d.n_tasks, B = S.rollout_B, T = S.rollout_T;
    const long long n_envs = (long long)M * B;
    if (s < 0 || s >= T) return fail(-1, "vectorised step %d outside [0, %d)", s, T);
    if (s < S.dev_filed) return fail(-3, "step %d has already been filed: every step is filed once, the next one is %d", s, S.dev_filed);
    if (s > S.dev_filed) return fail(-3, "step %d filed out of order: the next step to file is %d", s, S.dev_filed);
    if (s >= S.dev_policy_done)
        return fail(-3, "step %d filed before its policy step: promp_policy_step_dev has taken %d step(s)", s, S.dev_policy_done);
    if (S.rollout_ragged && max_path_length < 1) return fail(-1, "max_path_length = %d must be positive", max_path_length);
    if (n_envs * T > 0x7FFFFFFFll / 4) return fail(-1, "max_steps * environments = %lld staging rows are too many", n_envs * T);
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    FileStepArgs a;
    a.rewards = d_rewards; a.done = d_done; a.ended_out = d_ended_out;
    a.n_envs = (int)n_envs; a.s = s; a.max_path_length = max_path_length;
    if (S.rollout_ragged) {
        if (s == 0) {                  // a collection's storage is reserved by its first filing and stays put until the next one's
            if (c->dev_rew_stage.reserve((size_t)T * n_envs, 1)) return -2;
            if (c->dev_tables.reserve(dev_collect_views(c, T, n_envs).n_int, 1)) return -2;
            if (c->dev_stop.reserve(4, 1)) return -2;
        }
        const DevCollectViews v = dev_collect_views(c, T, n_envs);
        a.rew_out = c->dev_rew_stage.p + (size_t)s * n_envs; a.rew_env_stride = 1;
        a.end_len = v.end_len + (size_t)s * n_envs; a.ep_len = v.ep_len; a.fixed_end = 0;
    } else {                           // fixed horizon: slab row env * T + s, every episode ends with the last step
        a.rew_out = S.rew.p + s; a.rew_env_stride = T;
        a.end_len = nullptr; a.ep_len = nullptr; a.fixed_end = s == T - 1 ? 1 : 0;
    }
    if (producer_enter(c, producer_stream)) return -2;
    PROMP_LAUNCH(k_file_step, dim3((unsigned)((n_envs + 255) / 256)), 256, 0, c->stream, a);
    HIPCHECK(hipGetLastError());
    if (producer_leave(c, producer_stream)) return -2;
    S.dev_filed = s + 1;
    if (!S.rollout_ragged) { S.processed = false; S.has_rew64 = false; }
    return 0;
}

int promp_collection_progress(promp_ctx* c, int step, int64_t total_samples, int32_t* stop_step, int64_t* finished_rows) {
    if (!c || !stop_step || !finished_rows) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (const int rc = dev_collection_of(sc, "promp_collection_progress", total_samples)) return rc;
    StepData& S = sc.S();
    long long stop[3] = {-1, 0, 1};
    if (S.dev_filed > 0) {
        if (sc.open(/*writes=*/false, /*needs_data=*/false)) return sc.rc;
        if (dev_collect_stop(c, S, total_samples, stop)) return -2;
    }
    *stop_step = (int32_t)stop[0];
    *finished_rows = stop[1];
    return 0;
}

int promp_end_collection_dev(promp_ctx* c, int step, int64_t total_samples, int32_t* n_paths_out, int32_t* n_steps_out,
                             int32_t* task_path_offsets, int32_t* path_env, int32_t* path_start, int32_t* path_len) {
    if (!c || !n_paths_out || !n_steps_out || !task_path_offsets || !path_env || !path_start || !path_len) return fail(-1, "NULL argument");
    StepScope sc(c, step);
    if (const int rc = dev_collection_of(sc, "promp_end_collection_dev", total_samples)) return rc;
    StepData& S = sc.S();
    const int M = c->d.n_tasks, B = S.rollout_B, filed = S.dev_filed, max_paths = c->d.max_paths;
    const long long n_envs = (long long)M * B;
    if (filed < 1) return fail(-3, "promp_end_collection_dev: no step has been filed for step %d (promp_file_step_dev)", step);
    if (sc.open(/*writes=*/true, /*needs_data=*/false)) return sc.rc;
    hipStream_t st = c->stream;
    const DevCollectViews v = dev_collect_views(c, S.rollout_T, n_envs);
    long long stop[3] = {-1, 0, 1};
    if (dev_collect_stop(c, S, total_samples, stop)) return -2;
    if (stop[2] != 0 || stop[0] < 0)   // (nothing installed, the collection stays open: more steps may be filed)
        return fail(-1, "the %d vectorised steps filed do not reach total_samples = %lld", filed, (long long)total_samples);
    if (stop[1] > c->d.max_rows) return fail(-1, "%lld collected rows exceed max_rows = %d", stop[1], c->d.max_rows);
    CollectTablesArgs ct;
    ct.end_len = v.end_len; ct.stop = c->dev_stop; ct.task_count = v.count; ct.task_path_offsets = v.tpo;
    ct.path_env = v.env; ct.path_start = v.start; ct.path_len = v.len;
    ct.B = B; ct.max_steps = filed; ct.n_envs = (int)n_envs; ct.n_tasks = M; ct.max_paths = max_paths; ct.write = 0;
    PROMP_LAUNCH(k_collect_tables, dim3(M), 64, 0, st, ct);
    PROMP_LAUNCH(k_collect_offsets, dim3(1), 64, 0, st, (const int*)v.count, v.tpo, M);
    ct.write = 1;
    PROMP_LAUNCH(k_collect_tables, dim3(M), 64, 0, st, ct);
    HIPCHECK(hipGetLastError());
    std::vector<int32_t> tpo((size_t)M + 1, 0);
    HIPCHECK(hipMemcpyAsync(tpo.data(), v.tpo, sizeof(int32_t) * (M + 1), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    const int n_paths = tpo[M];
    if (n_paths < 1 || n_paths > max_paths) return fail(-1, "%d paths outside [1, max_paths = %d]", n_paths, max_paths);
    std::string empty;
    for (int i = 0; i < M; ++i)
        if (tpo[i + 1] == tpo[i]) empty += (empty.empty() ? "" : ", ") + std::to_string(i);
    if (!empty.empty())
        return fail(-1, "no finished episode for task(s) [%s] within total_samples = %lld (envs_per_task = %d)", empty.c_str(),
                    (long long)total_samples, B);
    // (the caller's tables are written only once the collection is accepted)
    std::vector<int32_t> h_env((size_t)n_paths), h_start((size_t)n_paths), h_len((size_t)n_paths), pro((size_t)n_paths + 1, 0);
    HIPCHECK(hipMemcpyAsync(h_env.data(), v.env, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h_start.data(), v.start, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h_len.data(), v.len, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int p = 0; p < n_paths; ++p) {
        if (h_len[p] < 1 || h_start[p] < 0 || h_start[p] + h_len[p] > filed || h_env[p] < 0 || h_env[p] >= n_envs)
            return fail(-2, "path %d (environment %d, steps [%d, %d)) lies outside the collection", p, h_env[p], h_start[p], h_start[p] + h_len[p]);
        pro[p + 1] = pro[p] + h_len[p];
    }
    if (pro[n_paths] != stop[1]) return fail(-2, "the path tables hold %d rows, the stop record %lld", pro[n_paths], stop[1]);
    if (finish_collection(sc, n_paths, tpo.data(), pro.data(), nullptr, nullptr, v.env, v.start, nullptr, c->dev_rew_stage)) return -2;
    S.dev_policy_done = S.dev_filed = 0;
    for (int i = 0; i <= M; ++i) task_path_offsets[i] = tpo[i];
    for (int p = 0; p < n_paths; ++p) { path_env[p] = h_env[p]; path_start[p] = h_start[p]; path_len[p] = h_len[p]; }
    *n_paths_out = n_paths;
    *n_steps_out = (int32_t)stop[0] + 1;
    return 0;
}

int promp_upload_step_dev(promp_ctx* c, int step, int n_paths, const int32_t* tpo, const int32_t* pro, const float* obs,
                          const float* act, const float* rew, const float* old_mean, const float* old_ls, int ls_per_row,
                          void* producer_stream) {
    NEED_CTX(c);
    if (check_dev_ptr("promp_upload_step_dev: obs", obs) || check_dev_ptr("promp_upload_step_dev: rew", rew)) return -1;
    if (act && old_mean && old_ls &&
        (check_dev_ptr("promp_upload_step_dev: act", act) || check_dev_ptr("promp_upload_step_dev: old_mean", old_mean) ||
         check_dev_ptr("promp_upload_step_dev: old_log_std", old_ls)))
        return -1;
    StepScope sc(c, step, /*writes=*/true, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    clear_selection(c, step);
    if (set_step_layout(c, S, c->stream, false, n_paths, tpo, pro)) return -2;
    if (producer_enter(c, producer_stream)) return -2;
    if (copy_step_data(c, S, c->stream, obs, act, rew, old_mean, old_ls, ls_per_row, hipMemcpyDeviceToDevice)) return -2;
    return producer_leave(c, producer_stream);
}

int promp_download_step(promp_ctx* c, int step, float* obs, float* act, float* rew, float* old_mean, float* old_log_std) {
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/true);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    const size_t R = S.n_rows, O = c->d.obs_dim, A = c->d.act_dim, M = c->d.n_tasks;
    hipStream_t st = c->stream;
    if (obs) HIPCHECK(hipMemcpyAsync(obs, S.obs, sizeof(float) * R * O, hipMemcpyDeviceToHost, st));
    if (rew) HIPCHECK(hipMemcpyAsync(rew, S.rew, sizeof(float) * R, hipMemcpyDeviceToHost, st));
    if ((act || old_mean || old_log_std) && !S.has_policy) return fail(-3, "step %d holds no actions / agent_infos", step);
    if (act) HIPCHECK(hipMemcpyAsync(act, S.act, sizeof(float) * R * A, hipMemcpyDeviceToHost, st));
    if (old_mean) HIPCHECK(hipMemcpyAsync(old_mean, S.old_mean, sizeof(float) * R * A, hipMemcpyDeviceToHost, st));
    if (old_log_std) HIPCHECK(hipMemcpyAsync(old_log_std, S.old_ls, sizeof(float) * (S.ls_per_row ? R : M) * A, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

int promp_meta_grad(promp_ctx* c, float clip_eps, const float* eta, int inner_kind, int outer_kind, float* grad_out,
                    float* stats_out) {
    if (!c || !eta) return fail(-1, "NULL argument");
    EvalSet E = full_set(c);
    if (c->use_sel && outer_kind == PROMP_OUTER_KL) {        // the constraint on the selections (promp_use_selection)
        const int rc = selection_set(c, inner_kind, &E);
        if (rc) return rc;
    }
    if (upload_eta(c, eta)) return -2;
    if (enqueue_meta_on(c, E, clip_eps, eta, inner_kind, outer_kind, true, false, 0.f, true)) return -2;
    if (grad_out && params_out(c, grad_out, c->grad_mean, 1)) return -2;
    if (stats_out && copy_out(c, stats_out, c->stats, c->d.num_inner_steps + 2)) return -2;
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// Exact Hessian-vector product of the TRPO constraint, mean_i KL(pi_old || pi_{theta'_i(theta)}) on the last step's samples,
// through the adaptation: with J_k = I - diag(alpha) H_k(theta_k) (H_k = Hessian of task i's inner objective on step k),
//     H v = mean_i  J_0^T ... J_{K-1}^T  H_KL(theta_K)  J_{K-1} ... J_0  v .
// The terms that differentiate the J_k are contracted with grad_{theta_K} KL, which is zero where TRPO builds the
// product: at the parameters the samples were drawn with (old distribution == adapted policy).  2K + 1 R-operator passes.
// (the direction is in c->grad_mean, the sums over the tasks -- all-reduced -- are left in c->red)
static int enqueue_constraint_hvp(promp_ctx* c, const EvalSet& E, int inner_kind, int refresh_chain) {
    PassSlab* const* W = E.slab;
    ChvpRec& R = *E.chvp;
    if (sharded_without_comm(c))
        return fail(-3, "this context holds %d of %d tasks and has no communicator: the product would be this rank's share only "
                        "(promp_comm_init first)", c->d.n_tasks, c->d.n_tasks_global);
    const int K = c->d.num_inner_steps, M = c->d.n_tasks, NP = c->NP;
    const size_t MNP = (size_t)M * NP;
    for (int k = 0; k <= K; ++k) {
        if (W[k]->n_rows == 0) return fail(-3, "step %d has no data", k);
        if (E.full && join_side(c, E.full[k])) return -2;
    }
    if (!c->wbuf && c->wbuf.alloc(MNP)) return -2;
    auto theta_of = [&](int k, long long* stride) -> const float* {
        *stride = (k == 0) ? 0 : NP;
        return (k == 0) ? c->theta : E.chain + (size_t)k * MNP;
    };
    const int lk = loss_kind_inner(inner_kind);
    long long st = 0;
    // Primal caches: the products of one conjugate-gradient solve all run at the same parameters on the same slabs, so the
    // passes that refresh the chain store their activations (and one extra storing pass with the KL objective covers step K);
    // every R-operator pass below then reads them back instead of recomputing layers 1 and 2.  Same worth-it rule as the
    // meta-objective's cache (enqueue_meta).
    const bool use_cache = primal_cache_on(c);
    if (refresh_chain) {
        R.valid = false;
        for (int k = 0; k <= K && use_cache; ++k)
            if (ensure_primal_cache(c, *W[k])) return -2;
        for (int k = 0; k < K; ++k) {
            const float* th = theta_of(k, &st);
            if (k == 0 && E.full && adapt0_stands(c, inner_kind, use_cache)) {       // promp_inner_adapt has just run exactly this pass
                c->adapt_passes_skipped += 1;
                continue;
            }
            PassReq q;
            q.theta = th; q.theta_stride = st; q.loss_kind = lk; q.clip_ls = k == 0;
            q.red_mode = RED_STEP; q.cur = th; q.cur_stride = st; q.next = E.chain + (size_t)(k + 1) * MNP; q.scal = E.scal_inner + (size_t)k * M * 2;
            q.cache = use_cache ? 1 : 0;
            if (launch_pass(c, *W[k], q)) return -2;
        }
        if (use_cache) {
            PassReq q;
            q.theta = theta_of(K, &q.theta_stride); q.loss_kind = LOSS_KL; q.clip_ls = K == 0; q.cache = 1;
            if (launch_pass(c, *W[K], q)) return -2;
            R.valid = true; R.theta_version = c->theta_version; R.sizes_version = c->sizes_version;
            R.inner_kind = inner_kind; R.min_log_std = c->min_log_std;
            for (int k = 0; k <= K; ++k) {
                R.data_version[k] = W[k]->data_version;
                R.tag[k] = W[k]->cache_tag;
            }
        }
    }
    const bool rec_ok = use_cache && R.valid && R.theta_version == c->theta_version && R.sizes_version == c->sizes_version &&
                        R.inner_kind == inner_kind && R.min_log_std == c->min_log_std;
    auto cache_ok = [&](int k) {
        return rec_ok && W[k]->hcache && R.data_version[k] == W[k]->data_version && R.tag[k] == W[k]->cache_tag;
    };
    PROMP_LAUNCH(k_replicate, dim3((NP + 255) / 256), 256, 0, c->stream, c->vbuf, c->grad_mean, NP, M);
    const dim3 eg((NP + 255) / 256, M);
    auto pass = [&](int k, int kind) -> int {
        PassReq q;
        q.hvp = true; q.theta = theta_of(k, &q.theta_stride); q.loss_kind = kind; q.clip_ls = k == 0;
        q.cache = cache_ok(k) ? 2 : 0;
        c->chvp_cached_passes += q.cache ? 1 : 0;
        return launch_pass(c, *W[k], q);
    };
    for (int k = 0; k < K; ++k) {                      // u = J_{K-1} ... J_0 v
        if (pass(k, lk)) return -2;
        PROMP_LAUNCH(k_jstep, eg, 256, 0, c->stream, c->vbuf, c->wbuf, c->lam, c->step_sizes, NP, 0);
    }
    if (pass(K, LOSS_KL)) return -2;                   // w = H_KL(theta_K) u
    PROMP_LAUNCH(k_jstep, eg, 256, 0, c->stream, c->vbuf, c->wbuf, c->lam, c->step_sizes, NP, 1);
    for (int k = K - 1; k >= 0; --k) {                 // w = J_k^T w
        if (pass(k, lk)) return -2;
        PROMP_LAUNCH(k_jstep, eg, 256, 0, c->stream, c->vbuf, c->wbuf, c->lam, c->step_sizes, NP, 2);
    }
    HIPCHECK(hipGetLastError());
    FinalArgs f;
    f.lam = c->wbuf; f.NP = NP; f.K = K; f.n_tasks = M;
    f.scal_inner = E.scal_inner; f.scal_outer = c->scal_outer; f.red = c->red; f.want_grad = 1;
    c->red_has_sizes = false;
    if (launch_final_stage(c, final_launch(c, false, true, false), &f, nullptr)) return -2;
    if (exchange_sums(c, c->red, (size_t)NP)) return -4;
    for (int k = 0; k <= K && E.full; ++k) E.full[k].dirty = true;
    return 0;
}

int promp_constraint_hvp(promp_ctx* c, int inner_kind, const float* v, int refresh_chain, float* out) {
    if (!c || !v || !out) return fail(-1, "NULL argument");
    EvalSet E = full_set(c);
    if (c->use_sel) {
        const int rc = selection_set(c, inner_kind, &E);
        if (rc) return rc;
    }
    if (params_in(c, c->grad_mean, v, 1)) return -2;
    const int rc = enqueue_constraint_hvp(c, E, inner_kind, refresh_chain);
    if (rc) return rc;
    if (params_out(c, out, c->red, 1)) return -2;
    const float inv = 1.0f / (float)c->d.n_tasks_global;
    for (int j = 0; j < c->NPu; ++j) out[j] *= inv;
    return 0;
}

// ConjugateGradientOptimizer's solve with nothing crossing to the host between its products (conjugate_gradient_optimizer.py:325-354
// conjugate_gradients(), :59-104 FiniteDifferenceHvp.Hx / build_eval, :259-264 the solve and the closing product): see include/promp_hip.h.
int promp_cg_solve(promp_ctx* c, int inner_kind, const float* b, int cg_iters, float reg_coeff, float eps, int hvp_mode,
                   float residual_tol, float* x_out, double* xhx_out) {
    if (!c || !b || !x_out || !xhx_out) return fail(-1, "NULL argument");
    if (cg_iters < 0) return fail(-1, "cg_iters must not be negative");
    if (hvp_mode < 0 || hvp_mode > 2) return fail(-1, "hvp_mode %d unknown (0 symmetric differences, 1 one-sided, 2 exact)", hvp_mode);
    if (hvp_mode != 2 && !(eps > 0.f)) return fail(-1, "the finite differences need eps > 0");
    if (sharded_without_comm(c))
        return fail(-3, "this context holds %d of %d tasks and has no communicator: the products would be this rank's share only "
                        "(promp_comm_init first)", c->d.n_tasks, c->d.n_tasks_global);
    // every step has a selection: the products run on the compact slabs; some have one: refused before anything is written
    EvalSet E = full_set(c);
    if (n_selected(c) > 0) {
        const int rc = selection_set(c, inner_kind, &E);
        if (rc) return rc;
    }
    const int NP = c->NP;
    // (one guard each: a call whose second allocation failed must not leave the next one running k_cg_step without its scalars)
    if (!c->cg_buf && c->cg_buf.alloc((size_t)7 * NP)) return -2;
    if (!c->cg_scal && c->cg_scal.alloc(4)) return -2;
    float *x = c->cg_buf, *r = x + NP, *d = r + NP, *hd = d + NP, *ga = hd + NP, *th0 = ga + NP;
    if (params_in(c, r, b, 1)) return -2;                       // (blocking: b is the caller's)
    float eta[PROMP_ETA_MAX] = {};
    if (upload_eta(c, eta)) return -2;
    CgArgs a;
    a.g_ahead = ga; a.g_behind = nullptr; a.div_h = 1.f; a.mul_s = 1.f; a.reg = reg_coeff;
    a.x = x; a.r = r; a.d = d; a.hd = hd; a.scal = c->cg_scal; a.tol = residual_tol; a.n = NP; a.mode = 2;
    PROMP_LAUNCH(k_cg_step, dim3(1), 1024, 0, c->stream, a);      // x = 0, d = r = b, scal = {b.b, 0, 0, 0}
    HIPCHECK(hipGetLastError());
    const bool exact = hvp_mode == 2;
    const bool ls_known = c->ls_known;
    auto gradient_at = [&](float s, const float* v) -> int {      // the constraint's gradient at theta0 + s v -> c->grad_mean
        PROMP_LAUNCH(k_cg_displace, dim3((NP + 255) / 256), 256, 0, c->stream, c->theta, th0, v, s, NP);
        c->theta_version = ++c->version_counter;
        c->ls_known = false;
        return enqueue_meta_on(c, E, 0.f, eta, inner_kind, PROMP_OUTER_KL, true, false, 0.f, /*sizes_grad=*/false);
    };
    if (!exact) {
        HIPCHECK(hipMemcpyAsync(th0, c->theta, sizeof(float) * NP, hipMemcpyDeviceToDevice, c->stream));
        if (hvp_mode == 1) {                                      // one-sided: the gradient at theta0 itself, once
            if (enqueue_meta_on(c, E, 0.f, eta, inner_kind, PROMP_OUTER_KL, true, false, 0.f, /*sizes_grad=*/false)) return -2;
            HIPCHECK(hipMemcpyAsync(th0 + NP, c->grad_mean, sizeof(float) * NP, hipMemcpyDeviceToDevice, c->stream));
        }
    }
    bool fresh = false;
    auto product = [&](const float* v, int mode) -> int {        // hd = (H + reg I) v and the vector updates of `mode`
        if (exact) {
            HIPCHECK(hipMemcpyAsync(c->grad_mean, v, sizeof(float) * NP, hipMemcpyDeviceToDevice, c->stream));
            const int rc = enqueue_constraint_hvp(c, E, inner_kind, fresh ? 0 : 1);
            if (rc) return rc;
            fresh = true;
            a.g_ahead = c->red; a.g_behind = nullptr; a.div_h = 1.f; a.mul_s = 1.0f / (float)c->d.n_tasks_global;
        } else {
            if (gradient_at(eps, v)) return -2;
            HIPCHECK(hipMemcpyAsync(ga, c->grad_mean, sizeof(float) * NP, hipMemcpyDeviceToDevice, c->stream));
            if (hvp_mode == 0) {
                if (gradient_at(-eps, v)) return -2;
                a.g_behind = c->grad_mean; a.div_h = 2.f * eps;
            } else {
                a.g_behind = th0 + NP; a.div_h = eps;
            }
            a.g_ahead = ga; a.mul_s = 1.f;
        }
        a.mode = mode;
        PROMP_LAUNCH(k_cg_step, dim3(1), 1024, 0, c->stream, a);
        HIPCHECK(hipGetLastError());
        return 0;
    };
    int rc = 0;
    for (int it = 0; it < cg_iters && !rc; ++it) rc = product(d, 0);
    if (!rc) rc = product(x, 1);                                  // x . (H + reg I) x: the step length's denominator
    if (!exact) {                                                 // the parameters are back at theta0 when the solve returns
        HIPCHECK(hipMemcpyAsync(c->theta, th0, sizeof(float) * NP, hipMemcpyDeviceToDevice, c->stream));
        c->theta_version = ++c->version_counter;
        c->ls_known = ls_known;
    }
    if (rc) return rc;
    if (params_out(c, x_out, x, 1)) return -2;
    double sc[4];
    HIPCHECK(hipMemcpyAsync(sc, c->cg_scal, sizeof sc, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    *xhx_out = sc[3];
    return 0;
}

int promp_adam_step(promp_ctx* c, float lr) {
    NEED_CTX(c);
    // red still holds the (all-reduced) sums of the last promp_meta_grad
    if (c->train_sizes && !c->red_has_sizes)
        return fail(-3, "promp_adam_step: the step sizes are trained, but the exchange buffer holds no step-size gradient: the last "
                        "evaluation ran with the flag off, or was promp_constraint_hvp / promp_cg_solve (promp_meta_grad first)");
    // the split route's second half, on its own
    AdamArgs ad = adam_args(c, c->stats, c->eta_last, false, true);
    ad.lr_t = outer_step_begins(c, c->train_sizes, lr);
    return launch_final_stage(c, final_launch(c, true, true, c->train_sizes), nullptr, &ad);
}

// MAMLFirstOrderOptimizer's tf_optimizer_cls(**tf_optimizer_args) and max_grad_norm (include/promp_hip.h).  Validated in the plan
// (outer_opt_plan) before anything is touched; a new rule starts from zeroed slots and step count, new arguments keep them.
int promp_set_outer_optimizer(promp_ctx* c, int rule, const float* args, float max_grad_norm) {
    NEED_CTX(c);
    OuterOptPlan p;
    std::string why;
    if (const int rc = outer_opt_plan(rule, args, max_grad_norm, &p, &why)) return fail(rc, "promp_set_outer_optimizer: %s", why.c_str());
    if (p.max_norm > 0.f && !c->grad_norm && c->grad_norm.alloc(1)) return -2;      // (a context that never clips allocates what it always did)
    if (p.rule != c->outer.rule) {
        const size_t bytes = sizeof(float) * (size_t)c->NP;
        HIPCHECK(hipMemsetAsync(c->adam_m, 0, bytes, c->stream));
        HIPCHECK(hipMemsetAsync(c->adam_v, 0, bytes, c->stream));
        if (c->ss_m) {
            HIPCHECK(hipMemsetAsync(c->ss_m, 0, bytes, c->stream));
            HIPCHECK(hipMemsetAsync(c->ss_v, 0, bytes, c->stream));
        }
        c->adam_t = 0;
    }
    if (!(p.max_norm > 0.f)) c->norm_valid = false;
    c->outer = p;
    return 0;
}
int promp_get_outer_optimizer(promp_ctx* c, int* rule, float* args, float* max_grad_norm) {
    NEED_CTX(c);
    outer_opt_unplan(c->outer, rule, args, max_grad_norm);
    return 0;
}
int promp_get_grad_norm(promp_ctx* c, float* out) {
    if (!c || !out) return fail(-1, "NULL argument");
    if (!(c->outer.max_norm > 0.f)) return fail(-3, "promp_get_grad_norm: gradient clipping is off (promp_set_outer_optimizer with max_grad_norm > 0)");
    if (!c->norm_valid) return fail(-3, "promp_get_grad_norm: no clipped step has been taken yet");
    return copy_out(c, out, c->grad_norm, 1);
}

int promp_optimize_begin(promp_ctx* c, int num_epochs, float lr, float clip_eps, const float* eta, int inner_kind, int outer_kind) {
    if (!c || !eta) return fail(-1, "NULL argument");
    if (num_epochs < 0) return fail(-1, "num_epochs must be >= 0");
    if (c->opt_pending) return fail(-1, "promp_optimize_begin: the previous optimisation has not been collected (promp_optimize_end)");
    if (sharded_without_comm(c)) return refuse_sharded_optimize(c);
    if (upload_eta(c, eta)) return -2;
    const int K = c->d.num_inner_steps;
    for (int e = 0; e < num_epochs; ++e) {
        // the loss evaluated by the first epoch, before its update, stays on the device (second statistics slot) until the
        // end: a download here would hold the host back until the epoch has run, and the next one would start late
        c->stats_slot = (e == 0) ? 1 : 0;
        const int rc = enqueue_meta(c, clip_eps, eta, inner_kind, outer_kind, true, true, lr);
        c->stats_slot = 0;
        if (rc) return -2;
    }
    // compute_stats.  Its final launch stores both statistics slots into page-locked host memory and then a sequence number
    // (system-scope release): no copy operation and no event on the queue, and nothing waits here -- the host can enqueue
    // the next batch's sample processing while this optimisation still runs
    c->stats_seq += 1;
    c->publish_next = true;
    const int rc_stats = enqueue_meta(c, clip_eps, eta, inner_kind, outer_kind, false, false, 0.f);
    c->publish_next = false;
    if (rc_stats) return -2;
    (void)K;
    c->opt_pending = true;
    c->opt_epochs = num_epochs;
    c->opt_theta_version = c->theta_version;
    return 0;
}

int promp_optimize_end(promp_ctx* c, float* loss_before, float* stats_after) {
    NEED_CTX(c);
    if (!c->opt_pending) return fail(-1, "promp_optimize_end without promp_optimize_begin");
    c->opt_pending = false;
    c->mb_enqueued = false;            // (returns behind the last launch or with the stream's error: nothing reads the staging any more)
    // poll the sequence number (the stream is queried now and then: a failed launch must not turn into an endless wait)
    for (unsigned long long spins = 0;; ++spins) {
        if (__atomic_load_n(c->stats_seq_host.p, __ATOMIC_ACQUIRE) == c->stats_seq) break;
        if ((spins & 0xfff) == 0xfff) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(c->stats_seq_host.p, __ATOMIC_ACQUIRE) == c->stats_seq) break;
                return fail(-2, "promp_optimize_end: the stream drained without publishing the statistics");
            }
            if (q != hipErrorNotReady) return fail(-2, "promp_optimize_end: %s", hipGetErrorString(q));
        }
    }
    const int K = c->d.num_inner_steps;
    // the smallest log_std entry the publishing launch saw: current only if nothing replaced theta between begin and end
    // (promp_set_theta / promp_adam_step in the window leave it unknown, as they do anywhere else)
    if (c->theta_version == c->opt_theta_version) {
        c->ls_min = c->stats_host[2 * (K + 2)];
        c->ls_known = true;
    }
    if (stats_after) memcpy(stats_after, c->stats_host, sizeof(float) * (K + 2));
    if (loss_before) *loss_before = c->opt_epochs > 0 ? c->stats_host[K + 2] : c->stats_host[0];
    return 0;
}

int promp_optimize(promp_ctx* c, int num_epochs, float lr, float clip_eps, const float* eta, int inner_kind, int outer_kind,
                   float* loss_before, float* stats_after) {
    if (promp_optimize_begin(c, num_epochs, lr, clip_eps, eta, inner_kind, outer_kind)) return -2;
    return promp_optimize_end(c, loss_before, stats_after);
}

int promp_optimize_minibatch_begin(promp_ctx* c, int num_epochs, int num_minibatches, const int32_t* assign, float lr, float clip_eps,
                                   const float* eta, int inner_kind, int outer_kind) {
    if (!c || !eta) return fail(-1, "NULL argument");
    const int E = num_epochs, B = num_minibatches;
    if (B < 1) return fail(-1, "num_minibatches %d is below 1", B);
    // one minibatch is the whole batch: today's call on today's path (and so is an optimisation of no epochs)
    if (B == 1 || E <= 0) return promp_optimize_begin(c, E, lr, clip_eps, eta, inner_kind, outer_kind);
    if (!assign) return fail(-1, "NULL argument");
    if (c->opt_pending) return fail(-1, "promp_optimize_minibatch_begin: the previous optimisation has not been collected (promp_optimize_end)");
    if (sharded_without_comm(c)) return refuse_sharded_optimize(c);
    if (inner_kind == PROMP_INNER_DICE)
        return fail(-3, "the DiCE inner objective is not evaluated on minibatches: the coupling rows of a path are not among the copies");
    const int K = c->d.num_inner_steps, M = c->d.n_tasks;
    for (int k = 0; k <= K; ++k) {
        const StepData& P = c->steps[k];
        if (P.n_rows == 0 || (int)P.lay_tpo.size() != M + 1) return fail(-3, "step %d has no data", k);
        if (P.has_dice) return fail(-3, "step %d carries DiCE rewards: minibatches are not formed of such steps (the coupling rows are not among the copies)", k);
        if (!P.has_policy) return fail(-3, "step has no actions / agent_infos uploaded");
        if (!P.has_adv) return fail(-3, "step has no advantages: call promp_process_samples or promp_set_advantages first");
    }
    // every epoch's partition of every step, before anything is allocated or enqueued
    std::vector<PartitionLayout> parts((size_t)E * (K + 1));
    {
        std::string why;
        const int32_t* a = assign;
        for (int e = 0; e < E; ++e)
            for (int k = 0; k <= K; ++k) {
                const StepData& P = c->steps[k];
                if (const int rc = build_partition(c->n_cus, c->max_work, M, P.n_paths, P.lay_tpo.data(), P.lay_pro.data(), B, a,
                                                   &parts[(size_t)e * (K + 1) + k], &why))
                    return fail(rc, "epoch %d, step %d: %s", e, k, why.c_str());
                a += P.n_paths;
            }
    }
    if (c->mb_enqueued) {              // (an earlier call gave up half-way: its copies may still read the staging)
        HIPCHECK(hipStreamSynchronize(c->stream));
        c->mb_enqueued = false;
    }
    size_t stage_ints = 0;
    if (mb_reserve(c, E, B, parts, &stage_ints)) return -2;
    if (upload_eta(c, eta)) return -2;
    c->mb_enqueued = true;
    // loss_before: the whole batch's objective at the parameters the first step starts from, parked in the second slot
    c->stats_slot = 1;
    const int rc_before = enqueue_meta(c, clip_eps, eta, inner_kind, outer_kind, false, false, 0.f);
    c->stats_slot = 0;
    if (rc_before) return -2;
    int* stage = c->mb_stage;
    for (int e = 0; e < E; ++e) {
        for (int k = 0; k <= K; ++k) {
            if (mb_enqueue_step(c, k, B, parts[(size_t)e * (K + 1) + k], stage)) return -2;
            stage += TableBlock(c->steps[k].n_paths, B, M, c->max_work).total;
        }
        for (int j = 0; j < B; ++j) {
            EvalSet S{{}, nullptr, c->mb_chain, c->mb_scal_inner, &c->chvp_mb};
            for (int k = 0; k <= K; ++k) S.slab[k] = &c->mb[k][j];
            if (enqueue_meta_on(c, S, clip_eps, eta, inner_kind, outer_kind, true, true, lr, true)) return -2;
        }
    }
    // compute_stats on the whole batch, publishing both slots (promp_optimize_begin)
    c->stats_seq += 1;
    c->publish_next = true;
    const int rc_stats = enqueue_meta(c, clip_eps, eta, inner_kind, outer_kind, false, false, 0.f);
    c->publish_next = false;
    if (rc_stats) return -2;
    c->opt_pending = true;
    c->opt_epochs = E;
    c->opt_theta_version = c->theta_version;
    return 0;
}

int promp_optimize_minibatch(promp_ctx* c, int num_epochs, int num_minibatches, const int32_t* assign, float lr, float clip_eps,
                             const float* eta, int inner_kind, int outer_kind, float* loss_before, float* stats_after) {
    if (promp_optimize_minibatch_begin(c, num_epochs, num_minibatches, assign, lr, clip_eps, eta, inner_kind, outer_kind)) return -2;
    return promp_optimize_end(c, loss_before, stats_after);
}

int promp_eval_loss_grad(promp_ctx* c, int step, int kind, float clip_eps, int clip_ls, float* grads_out, float* loss_out,
                         float* kl_out) {
    StepScope sc(c, step);
    if (sc.rc) return sc.rc;
    if (kind < 0 || kind > 3) return fail(-1, "unknown objective kind %d", kind);
    if (sc.open(/*writes=*/false, /*needs_data=*/false)) return sc.rc;
    StepData& S = sc.S();
    const int M = c->d.n_tasks;
    if (tasks_materialize(c)) return -2;
    PassReq q;
    q.theta = c->theta_tasks; q.theta_stride = c->NP; q.loss_kind = kind; q.clip_eps = clip_eps; q.clip_ls = clip_ls;
    if (launch_pass(c, pass_slab(S), q)) return -2;
    if (grads_out && params_out(c, grads_out, c->lam, (size_t)M)) return -2;
    std::vector<float> scal((size_t)M * 2);
    if (copy_out(c, scal.data(), c->scal_tmp, scal.size())) return -2;
    for (int i = 0; i < M; ++i) {
        if (loss_out) loss_out[i] = scal[2 * i];
        if (kl_out) kl_out[i] = scal[2 * i + 1];
    }
    return 0;
}

int promp_eval_hvp(promp_ctx* c, int step, int inner_kind, int clip_ls, float klw, const float* v, float* out) {
    if (!c || !v || !out) return fail(-1, "NULL argument");
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    const int M = c->d.n_tasks, NP = c->NP;
    if (params_in(c, c->vbuf, v, (size_t)M)) return -2;
    HIPCHECK(hipMemsetAsync(c->lam, 0, sizeof(float) * (size_t)M * NP, c->stream));
    if (tasks_materialize(c)) return -2;
    PassReq q;
    q.hvp = true; q.theta = c->theta_tasks; q.theta_stride = NP; q.loss_kind = loss_kind_inner(inner_kind); q.clip_ls = clip_ls; q.klw = klw;
    if (launch_pass(c, pass_slab(S), q)) return -2;
    return params_out(c, out, c->lam, (size_t)M);
}

int promp_comm_unique_id(void* id_out, size_t id_bytes) {
    if (!id_out || id_bytes < sizeof(ncclUniqueId)) return fail(-1, "id buffer must hold %zu bytes", sizeof(ncclUniqueId));
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(-4, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    memset(id_out, 0, id_bytes);
    memcpy(id_out, &id, sizeof id);
    return 0;
}

int promp_comm_init(promp_ctx* c, int rank, int nranks, const void* id, size_t id_bytes) {
    NEED_CTX(c);
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(-1, "bad rank %d / nranks %d", rank, nranks);
    if (!id || id_bytes < sizeof(ncclUniqueId)) return fail(-1, "id buffer must hold %zu bytes", sizeof(ncclUniqueId));
    HIPCHECK(hipSetDevice(c->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, uid, rank);
    if (r != ncclSuccess) return fail(-4, "ncclCommInitRank failed: %s", ncclGetErrorString(r));
    c->rank = rank;
    c->nranks = nranks;
    return 0;
}

int promp_comm_info(promp_ctx* c, int32_t* nranks, int32_t* rank, int32_t* fixed_order, char* bus_id_out, size_t bus_id_bytes) {
    NEED_CTX(c);
    int n = 1, r = 0;
    if (c->comm) {        // what the communicator itself says, not what the caller passed to promp_comm_init
        ncclResult_t e = ncclCommCount(c->comm, &n);
        if (e == ncclSuccess) e = ncclCommUserRank(c->comm, &r);
        if (e != ncclSuccess) return fail(-4, "ncclCommCount / ncclCommUserRank failed: %s", ncclGetErrorString(e));
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (fixed_order) *fixed_order = c->fixed_order ? 1 : 0;
    if (bus_id_out && bus_id_bytes) {
        bus_id_out[0] = 0;
        HIPCHECK(hipDeviceGetPCIBusId(bus_id_out, (int)bus_id_bytes, c->device));
    }
    return 0;
}

int promp_comm_fixed_order(promp_ctx* c, int on) {
    NEED_CTX(c);
    c->fixed_order = on != 0;
    return 0;
}

int promp_comm_split_path(promp_ctx* c, int on) {
    NEED_CTX(c);
    c->force_split = on != 0;
    return 0;
}

int promp_comm_move(promp_ctx* dst, promp_ctx* src) {
    if (!dst || !src) return fail(-1, "ctx is NULL");
    if (dst == src) return 0;
    if (dst->comm) return fail(-3, "destination context already holds a communicator");
    if (dst->device != src->device) return fail(-1, "contexts live on different devices (%d, %d)", dst->device, src->device);
    HIPCHECK(hipStreamSynchronize(src->stream));    // nothing of the old context may still be using it
    dst->comm = src->comm;
    src->comm = nullptr;
    dst->fixed_order = src->fixed_order;
    dst->rank = src->rank; dst->nranks = src->nranks;
    src->rank = 0; src->nranks = 1;
    return 0;
}

int promp_reduced_get(promp_ctx* c, float* out) {
    if (!c || !out) return fail(-1, "NULL argument");
    // [grad Theta | K + 2 scalars]: the gradient part in the caller's layout, like every parameter vector that crosses the ABI
    if (params_out(c, out, c->red, 1)) return -2;
    const size_t ns = (size_t)c->d.num_inner_steps + 2;
    if (copy_out(c, out + c->NPu, c->red + c->NP, ns)) return -2;
    // trainable step sizes: [... | step-size gradient Theta], in the caller's layout as well
    return c->train_sizes ? params_out(c, out + c->NPu + ns, c->red + c->NP + ns, 1) : 0;
}
int promp_reduced_set(promp_ctx* c, const float* in) {
    if (!c || !in) return fail(-1, "NULL argument");
    if (params_in(c, c->red, in, 1)) return -2;
    const size_t ns = (size_t)c->d.num_inner_steps + 2;
    if (copy_in(c, c->red + c->NP, in + c->NPu, ns)) return -2;
    if (!c->train_sizes) return 0;
    if (params_in(c, c->red + c->NP + ns, in + c->NPu + ns, 1)) return -2;
    c->red_has_sizes = true;
    return 0;
}
int promp_reduced_count(promp_ctx* c) {
    NEED_CTX(c);
    return (c->train_sizes ? 2 : 1) * c->NPu + c->d.num_inner_steps + 2;
}

int promp_allreduce_f64(promp_ctx* c, double* buf, int n, int op) {
    if (!c || !buf) return fail(-1, "NULL argument");
    if (n < 1 || n > 64) return fail(-1, "n must be in [1,64]");
    if (c->nranks == 1) return 0;
    HIPCHECK(hipMemcpyAsync(c->red64, buf, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    ncclResult_t r = ncclAllReduce(c->red64, c->red64, (size_t)n, ncclDouble, op == 1 ? ncclMax : ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) return fail(-4, "ncclAllReduce failed: %s", ncclGetErrorString(r));
    HIPCHECK(hipMemcpyAsync(buf, c->red64, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// Developer tooling (not part of include/promp_hip.h): run one chain-kernel launch on the current per-task parameters
// with the cycle stamps of workgroup 0 enabled, and return the 256 raw stamps (needs a -DPROMP_DEV_STAMPS build).
int promp_debug_phase_stamps(promp_ctx* c, int step, int hvp, unsigned long long* out) {
    if (!c || !out) return fail(-1, "NULL argument");
    if (!PROMP_STAMPS_ON) return fail(-3, "phase stamps need a build with -DPROMP_DEV_STAMPS");
    StepScope sc(c, step, /*writes=*/false, /*needs_data=*/false);
    if (sc.rc) return sc.rc;
    StepData& S = sc.S();
    if (tasks_materialize(c)) return -2;
    PassReq q;
    q.theta = c->theta_tasks; q.theta_stride = c->NP; q.clip_eps = 0.3f;
    if (hvp == 2) {               // the cache-reading R-operator pass: fill the step's primal cache first (unstamped)
        if (c->family != PassFamily::Chain) return fail(-1, "no primal cache for this shape");
        if (ensure_primal_cache(c, pass_slab(S))) return -2;
        q.cache = 1;
        const int rc0 = launch_pass(c, pass_slab(S), q);
        if (rc0) return rc0;
    }
    HIPCHECK(hipMemsetAsync(c->dbg, 0, sizeof(unsigned long long) * (256 + 4 * 1024), c->stream));
    c->dbg_enabled = true;
    q.hvp = hvp != 0;
    q.cache = hvp == 2 ? 2 : 0;
    const int rc = launch_pass(c, pass_slab(S), q);
    c->dbg_enabled = false;
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(out, c->dbg, sizeof(unsigned long long) * (256 + 4 * 1024), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int promp_prof_enable(promp_ctx* c, int on) {
    NEED_CTX(c);
    if (prof_collect(c)) return -2;
    c->prof = on != 0;
    if (on)
        for (auto& s : c->prof_slots) { s.total_ms = 0.0; s.launches = 0; s.rows = 0; }
    return 0;
}

int promp_prof_read(promp_ctx* c, int id, double* total_ms, int64_t* launches, int64_t* rows) {
    NEED_CTX(c);
    if (id < 0 || id >= PROMP_KERNEL_COUNT) return fail(-1, "kernel id %d out of range", id);
    if (prof_collect(c)) return -2;
    if (total_ms) *total_ms = c->prof_slots[id].total_ms;
    if (launches) *launches = c->prof_slots[id].launches;
    if (rows) *rows = c->prof_slots[id].rows;
    return 0;
}

int promp_split_events(promp_ctx* c, int64_t* out2) {
    if (!c || !out2) return fail(-1, "NULL argument");
    int h[2];
    HIPCHECK(hipMemcpyAsync(h, c->split_events, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemsetAsync(c->split_events, 0, sizeof h, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 2; ++i) out2[i] = h[i];
    return 0;
}

int promp_device_info(promp_ctx* c, char* name_out, size_t name_bytes, int32_t* n_cus, int32_t* clock_mhz) {
    NEED_CTX(c);
    if (name_out && name_bytes) snprintf(name_out, name_bytes, "%s", c->dev_name);
    if (n_cus) *n_cus = c->n_cus;
    if (clock_mhz) *clock_mhz = c->clock_mhz;
    return 0;
}

}  // extern "C"
