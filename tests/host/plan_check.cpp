// plan_check.cpp -- the host planning of promp_amd/csrc/promp_plan.h, checked on the host alone.
//
// Stand-alone: includes the plan header and nothing else of the project.  tests/test_plan_host.py compiles it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined
// and runs it once.  One line per failed expectation, exit status 1 if there was any.
//
//   dispatch     every row of the kernel table in tests/test_gpu_parity.py's docstring gives exactly the kernels the table names
//   shapes       padded widths, remap_params round trip and where the zeros sit, Mlp2Layout against both; pass family and
//                observation class
//   step tables  the invariants the kernels rely on, for small, ragged, large and many-task layouts at 2, 8 and 256 CUs;
//                malformed offsets are refused with their message (and, under the sanitizer, without a stray access);
//                one item per task at 1 CU and the 256-row cut of 513 rows at 2 CUs (what tests/layered_checks.py builds on);
//                items, chain segments and workgroup offsets of the row cases of tests/fused_checks.py at 1 and 2 CUs
//   gramt        the wave -> square map of k_gram_tiled
#include "../../promp_amd/csrc/promp_plan.h"

#include <cstdio>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

static int g_failed = 0;
#define EXPECT(cond, ...)                                    \
    do {                                                     \
        if (!(cond)) {                                       \
            ++g_failed;                                      \
            printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                             \
            printf("\n");                                    \
        }                                                    \
    } while (0)

static promp_dims make_dims(int O, int A, std::vector<int> hidden, int act = PROMP_ACT_TANH) {
    promp_dims d;
    memset(&d, 0, sizeof d);
    d.n_tasks = d.n_tasks_global = 2;
    d.obs_dim = O; d.act_dim = A;
    d.n_hidden = (int)hidden.size();
    hidden.resize(4, 0);
    d.hidden1 = hidden[0]; d.hidden2 = hidden[1]; d.hidden3 = hidden[2]; d.hidden4 = hidden[3];
    d.num_inner_steps = 1; d.max_rows = 100; d.max_paths = 10;
    d.hidden_act = act;
    return d;
}

// ---- dispatch ------------------------------------------------------------------------------------------------------------
struct Row {
    int O, cols, nblk;           // obs_dim, D + 1, blocks of 16
    GramKernel gram;
    int gram_arg;                // Small: NBLK; Wide: pair slices; Tiled: slices of 16 squares
    FitKernel fit;
    int fit_arg;                 // Wave: DT; Wide: NB
    bool phases;
    bool untiled, one_launch;    // the switches the row is planned under
};
static void check_row(const Row& r, int kind = PROMP_BASELINE_LINEAR_FEATURE) {
    const promp_dims d = make_dims(r.O, 2, {32, 32});
    PlanSwitches sw;
    sw.gram_untiled = r.untiled;
    sw.fit_one_launch = r.one_launch;
    SamplePlan p;
    std::string why;
    const int D = feature_dim(&d, kind);
    const int rc = sample_plan(kind, r.O, D, sw, &p, &why);
    EXPECT(rc == 0, "obs %d: refused: %s", r.O, why.c_str());
    EXPECT(D + 1 == r.cols && p.nblk == r.nblk, "obs %d: %d columns in %d blocks, table says %d in %d", r.O, D + 1, p.nblk, r.cols, r.nblk);
    EXPECT(p.gram == r.gram, "obs %d untiled %d: Gram kernel %d, table says %d", r.O, (int)r.untiled, (int)p.gram, (int)r.gram);
    const int garg = p.gram == GramKernel::Small ? p.gram_nblk : p.gram_slices;
    EXPECT(garg == r.gram_arg, "obs %d untiled %d: Gram NBLK / slices %d, table says %d", r.O, (int)r.untiled, garg, r.gram_arg);
    EXPECT(p.fit == r.fit, "obs %d: fit kernel %d, table says %d", r.O, (int)p.fit, (int)r.fit);
    EXPECT(p.fit_arg == r.fit_arg, "obs %d: fit DT / NB %d, table says %d", r.O, p.fit_arg, r.fit_arg);
    EXPECT(p.fit_phases == r.phases, "obs %d one_launch %d: per-phase launches %d, table says %d", r.O, (int)r.one_launch, (int)p.fit_phases, (int)r.phases);
    if (p.gram == GramKernel::Wide) EXPECT(p.gram_rows == 64 || p.gram_rows == 32 || p.gram_rows == 16, "obs %d: %d rows per round", r.O, p.gram_rows);
    if (p.gram == GramKernel::Tiled) {
        EXPECT(p.gram_rows == 32 || p.gram_rows == 16, "obs %d: %d rows per round", r.O, p.gram_rows);
        EXPECT((size_t)(p.gram_db ? 2 : 1) * p.gram_rows * gramt_fs(p.nblk) * sizeof(double) <= 160 * 1024, "obs %d: feature tiles outgrow LDS", r.O);
    }
    if (p.fit == FitKernel::Wide) {
        EXPECT(fitw_smem(D, p.fit_arg) <= 160 * 1024, "obs %d: %zu bytes of LDS for the %d-column panel", r.O, fitw_smem(D, p.fit_arg), p.fit_arg);
        EXPECT(p.sum_split == (p.nblk >= 32 ? 32 : p.nblk >= 13 ? 16 : 8), "obs %d: sum split %d", r.O, p.sum_split);
    }
}
static void check_dispatch() {
    const GramKernel S = GramKernel::Small, W = GramKernel::Wide, T = GramKernel::Tiled;
    const FitKernel FW = FitKernel::Wave, FB = FitKernel::Block, FX = FitKernel::Wide;
    // squares of k_gram_tiled: bands nb = ceil(nblk / 3), nb (nb + 1) / 2 squares, 16 per slice:
    //   nblk 13: 5 bands, 15 squares, 1 slice | 17, 18: 6, 21, 2 | 25, 26: 9, 45, 3 | 35: 12, 78, 5 | 61: 21, 231, 15
    const Row rows[] = {
        {1, 7, 1, S, 1, FW, 12, false, false, false},     {3, 11, 1, S, 1, FW, 12, false, false, false},
        {4, 13, 1, S, 1, FW, 45, false, false, false},    {5, 15, 1, S, 1, FW, 45, false, false, false},
        {6, 17, 2, S, 2, FW, 45, false, false, false},    {13, 31, 2, S, 2, FW, 45, false, false, false},
        {14, 33, 3, S, 3, FW, 45, false, false, false},   {20, 45, 3, S, 3, FW, 45, false, false, false},
        {21, 47, 3, S, 3, FW, 48, false, false, false},
        {22, 49, 4, S, 4, FW, 64, false, false, false},   {29, 63, 4, S, 4, FW, 64, false, false, false},
        {30, 65, 5, S, 5, FB, 0, false, false, false},    {32, 69, 5, S, 5, FB, 0, false, false, false},
        {33, 71, 5, W, 1, FX, 32, false, false, false},
        {93, 191, 12, W, 1, FX, 32, false, false, false},
        {94, 193, 13, T, 1, FX, 32, false, false, false},
        {133, 271, 17, T, 2, FX, 32, false, false, false}, {133, 271, 17, W, 1, FX, 32, false, true, false},
        {134, 273, 18, T, 2, FX, 32, false, false, false}, {134, 273, 18, W, 2, FX, 32, false, true, false},
        {197, 399, 25, T, 3, FX, 32, false, false, false},
        {198, 401, 26, T, 3, FX, 32, true, false, false},  {198, 401, 26, T, 3, FX, 32, false, false, true},
        {274, 553, 35, T, 5, FX, 32, true, false, false},
        {275, 555, 35, T, 5, FX, 16, true, false, false},
        {480, 965, 61, T, 15, FX, 16, true, false, false},
    };
    for (const Row& r : rows) check_row(r);
    // LinearTimeBaseline reads no observations: four features at any obs_dim
    check_row({40, 5, 1, S, 1, FW, 12, false, false, false}, PROMP_BASELINE_LINEAR_TIME);
    {   // no baseline: no Gram, no fit
        SamplePlan p;
        std::string why;
        EXPECT(sample_plan(PROMP_BASELINE_ZERO, 481, 0, PlanSwitches(), &p, &why) == 0, "ZeroBaseline refused: %s", why.c_str());
        EXPECT(p.gram == GramKernel::None && p.fit == FitKernel::None, "ZeroBaseline plans kernels");
    }
    {   // one observation past PROMP_LINFEAT_MAX_O
        SamplePlan p;
        std::string why;
        EXPECT(sample_plan(PROMP_BASELINE_LINEAR_FEATURE, 481, 966, PlanSwitches(), &p, &why) == -1, "obs 481 accepted");
        const std::string want = "LinearFeatureBaseline's fit is sized for obs_dim <= 480 (481 here: 967 feature columns); fit LinearTimeBaseline / no "
                                 "baseline on the device, or hand advantages in through promp_set_advantages";
        EXPECT(why == want, "obs 481: message '%s'", why.c_str());
        EXPECT(sample_plan(PROMP_BASELINE_LINEAR_TIME, 481, 4, PlanSwitches(), &p, &why) == 0, "LinearTimeBaseline at obs 481 refused");
    }
}

// ---- shapes --------------------------------------------------------------------------------------------------------------
// (rows, cols) of the parameter blocks in the reference's order: per layer kernel then bias, output kernel and bias, log_std
static std::vector<std::pair<int, int>> param_blocks(int O, int A, const std::vector<int>& hidden) {
    std::vector<std::pair<int, int>> b;
    int in = O;
    for (int h : hidden) { b.push_back({in, h}); b.push_back({1, h}); in = h; }
    b.push_back({in, A}); b.push_back({1, A}); b.push_back({1, A});
    return b;
}
static void check_padding(int O, int A, const std::vector<int>& hidden, const std::vector<int>& padded) {
    const promp_dims du = make_dims(O, A, hidden);
    std::string why;
    EXPECT(check_dims(&du, &why) == 0, "obs %d hidden %d,..: refused: %s", O, hidden[0], why.c_str());
    promp_dims dp;
    pad_dims(&du, &dp);
    const int got[4] = {dp.hidden1, dp.hidden2, dp.hidden3, dp.hidden4};
    for (size_t l = 0; l < padded.size(); ++l) EXPECT(got[l] == padded[l], "obs %d hidden %d,..: layer %zu padded to %d, expected %d", O, hidden[0], l, got[l], padded[l]);
    EXPECT(dp.n_hidden == du.n_hidden && dp.obs_dim == O && dp.act_dim == A, "pad_dims changed more than the widths");
    // any other nonlinearity runs layer by layer at the widths given
    const promp_dims dr = make_dims(O, A, hidden, PROMP_ACT_RELU);
    promp_dims drp;
    pad_dims(&dr, &drp);
    EXPECT(memcmp(&dr, &drp, sizeof dr) == 0, "obs %d hidden %d,..: relu layers padded", O, hidden[0]);
    const auto bu = param_blocks(O, A, hidden), bp = param_blocks(O, A, padded);
    size_t nu = 0, np = 0;
    for (auto& b : bu) nu += (size_t)b.first * b.second;
    for (auto& b : bp) np += (size_t)b.first * b.second;
    EXPECT((size_t)param_count(&du) == nu && (size_t)param_count(&dp) == np, "obs %d hidden %d,..: param_count %d / %d, blocks say %zu / %zu", O,
           hidden[0], param_count(&du), param_count(&dp), nu, np);
    if (hidden.size() != 2) return;         // (remap_params serves the two-layer fused shapes; nothing else is ever padded)
    // exactly sized heap blocks: the sanitizer sees a write or a read one past either layout
    std::unique_ptr<float[]> v(new float[nu]), w(new float[np]()), back(new float[nu]());
    for (size_t i = 0; i < nu; ++i) v[i] = (float)(i + 1);
    remap_params(du, dp, v.get(), w.get(), true);
    size_t nonzero = 0;
    for (size_t i = 0; i < np; ++i) nonzero += w[i] != 0.f;
    EXPECT(nonzero == nu, "obs %d hidden %d,%d: %zu non-zero entries in the padded vector, %zu parameters", O, hidden[0], hidden[1], nonzero, nu);
    remap_params(du, dp, w.get(), back.get(), false);
    for (size_t i = 0; i < nu; ++i)
        if (back[i] != v[i]) { EXPECT(false, "obs %d hidden %d,%d: round trip changed entry %zu", O, hidden[0], hidden[1], i); break; }
    // the caller's block in the top-left corner of the padded block, zeros on the padded units
    size_t ou = 0, op = 0;
    for (size_t b = 0; b < bu.size(); ++b) {
        const int ru = bu[b].first, cu = bu[b].second, rp = bp[b].first, cp = bp[b].second;
        bool ok = true;
        for (int r = 0; r < rp && ok; ++r)
            for (int c = 0; c < cp && ok; ++c) {
                const float want = (r < ru && c < cu) ? v[ou + (size_t)r * cu + c] : 0.f;
                ok = w[op + (size_t)r * cp + c] == want;
            }
        EXPECT(ok, "obs %d hidden %d,%d: parameter block %zu is not the caller's block padded with zeros", O, hidden[0], hidden[1], b);
        ou += (size_t)ru * cu;
        op += (size_t)rp * cp;
    }
    // Mlp2Layout, the offsets every kernel indexes by: NP is param_count, the seven blocks follow each other without a gap in
    // remap_params' order, and a padded vector holds each caller entry at the offset the layout gives for the padded widths
    const Mlp2Layout lu = mlp2_layout(O, hidden[0], hidden[1], A), lp = mlp2_layout(O, padded[0], padded[1], A);
    const int offu[8] = {0, lu.b1, lu.W2, lu.b2, lu.W3, lu.b3, lu.ls, lu.NP}, offp[8] = {0, lp.b1, lp.W2, lp.b2, lp.W3, lp.b3, lp.ls, lp.NP};
    EXPECT(lu.NP == param_count(&du) && lp.NP == param_count(&dp), "obs %d hidden %d,%d: layout NP %d / %d, param_count %d / %d", O, hidden[0],
           hidden[1], lu.NP, lp.NP, param_count(&du), param_count(&dp));
    for (size_t b = 0; b < bu.size(); ++b) {
        EXPECT(offu[b + 1] - offu[b] == bu[b].first * bu[b].second && offp[b + 1] - offp[b] == bp[b].first * bp[b].second,
               "obs %d hidden %d,%d: layout block %zu spans %d / %d entries, the reference's order says %d / %d", O, hidden[0], hidden[1], b,
               offu[b + 1] - offu[b], offp[b + 1] - offp[b], bu[b].first * bu[b].second, bp[b].first * bp[b].second);
        bool ok = true;
        for (int r = 0; r < bu[b].first && ok; ++r)
            for (int c = 0; c < bu[b].second && ok; ++c)
                ok = w[offp[b] + (size_t)r * bp[b].second + c] == v[offu[b] + (size_t)r * bu[b].second + c];
        EXPECT(ok, "obs %d hidden %d,%d: block %zu of the padded vector is not at the layout's offset", O, hidden[0], hidden[1], b);
    }
}
static void check_family(int O, int A, const std::vector<int>& hidden, int act, PassFamily want, int cls, PassFamily want_fp32) {
    const promp_dims du = make_dims(O, A, hidden, act);
    std::string why;
    EXPECT(check_dims(&du, &why) == 0, "obs %d hidden %d,..: refused: %s", O, hidden[0], why.c_str());
    promp_dims dp;
    pad_dims(&du, &dp);
    PlanSwitches sw;
    FamilyPlan f = pass_family(&dp, sw);
    EXPECT(f.family == want && f.wb_cls == cls, "obs %d act %d hidden %d,..: family %d class %d, expected %d class %d", O, A, hidden[0], (int)f.family,
           f.wb_cls, (int)want, cls);
    sw.wide_fp32 = true;
    f = pass_family(&dp, sw);
    EXPECT(f.family == want_fp32 && f.wb_cls == (want_fp32 == PassFamily::CoopSplit ? cls : 0), "obs %d act %d hidden %d,.. with the FP32 switch: family %d class %d, expected %d",
           O, A, hidden[0], (int)f.family, f.wb_cls, (int)want_fp32);
}
static void check_refused(promp_dims d, const char* want) {
    std::string why;
    EXPECT(check_dims(&d, &why) == -1 && why == want, "check_dims: '%s', expected '%s'", why.c_str(), want);
}
static void check_shapes() {
    check_padding(20, 6, {100, 100}, {128, 128});
    check_padding(4, 2, {40, 40}, {64, 64});
    check_padding(5, 3, {20, 50}, {32, 64});
    check_padding(40, 3, {32, 32}, {64, 64});
    check_padding(20, 6, {64, 64}, {64, 64});
    check_padding(20, 6, {48, 48, 48}, {48, 48, 48});
    check_padding(10, 2, {16, 100}, {128, 128});
    check_padding(200, 4, {40, 40}, {40, 40});
    const PassFamily Chain = PassFamily::Chain, Fp32 = PassFamily::CoopFp32, Split = PassFamily::CoopSplit, Layered = PassFamily::Layered;
    for (int O : {1, 20, 32})
        for (int h1 : {32, 64})
            for (int h2 : {32, 64}) check_family(O, 6, {h1, h2}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(5, 3, {20, 50}, PROMP_ACT_TANH, Chain, 0, Chain);                 // padded to (32, 64)
    check_family(40, 6, {64, 64}, PROMP_ACT_TANH, Fp32, 0, Fp32);
    check_family(20, 6, {100, 100}, PROMP_ACT_TANH, Split, 1, Fp32);
    check_family(63, 6, {128, 128}, PROMP_ACT_TANH, Split, 1, Fp32);
    check_family(64, 6, {128, 128}, PROMP_ACT_TANH, Split, 2, Fp32);
    check_family(111, 8, {128, 128}, PROMP_ACT_TANH, Split, 2, Fp32);
    check_family(112, 8, {128, 128}, PROMP_ACT_TANH, Split, 3, Fp32);
    check_family(127, 8, {128, 128}, PROMP_ACT_TANH, Split, 3, Fp32);
    check_family(128, 8, {128, 128}, PROMP_ACT_TANH, Fp32, 0, Fp32);
    check_family(20, 6, {48, 48, 48}, PROMP_ACT_TANH, Layered, 0, Layered);
    check_family(20, 6, {256, 256}, PROMP_ACT_TANH, Layered, 0, Layered);
    check_family(20, 9, {64, 64}, PROMP_ACT_TANH, Layered, 0, Layered);
    check_family(20, 6, {64, 64}, PROMP_ACT_RELU, Layered, 0, Layered);
    check_family(129, 6, {64, 64}, PROMP_ACT_TANH, Layered, 0, Layered);
    // the shapes of tests/layered_checks.py: two tanh layers of up to 128 units with few actions are padded onto a fused family, the
    // same widths with nine actions (or a third layer) stay layer by layer -- which of its cases reach k_gb_* / k_gen_* hangs on this
    check_family(9, 3, {72, 40}, PROMP_ACT_TANH, Split, 1, Fp32);
    check_family(9, 9, {72, 40}, PROMP_ACT_TANH, Layered, 0, Layered);
    check_family(9, 3, {72, 40, 24}, PROMP_ACT_TANH, Layered, 0, Layered);
    check_family(33, 5, {33, 65}, PROMP_ACT_TANH, Split, 1, Fp32);
    check_family(33, 9, {33, 65}, PROMP_ACT_TANH, Layered, 0, Layered);
    check_family(5, 2, {33, 20}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(5, 9, {33, 20}, PROMP_ACT_TANH, Layered, 0, Layered);
    // the shapes of tests/fused_checks.py (ROW_SHAPES, DICE_SHAPES, RANGE_SHAPES, EMU_SHAPES), one per instantiation of the three
    // fused families: its cases reach the kernels they name only while these rows hold
    check_family(7, 3, {32, 32}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(20, 6, {32, 64}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(29, 8, {64, 32}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(32, 1, {64, 64}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(11, 7, {48, 20}, PROMP_ACT_TANH, Chain, 0, Chain);                // padded to (64, 32)
    check_family(9, 3, {32, 64}, PROMP_ACT_TANH, Chain, 0, Chain);
    check_family(33, 3, {64, 64}, PROMP_ACT_TANH, Fp32, 0, Fp32);
    check_family(64, 5, {64, 64}, PROMP_ACT_TANH, Fp32, 0, Fp32);
    check_family(111, 8, {64, 64}, PROMP_ACT_TANH, Fp32, 0, Fp32);
    check_family(40, 3, {48, 20}, PROMP_ACT_TANH, Fp32, 0, Fp32);                  // padded to (64, 64)
    check_family(40, 3, {64, 64}, PROMP_ACT_TANH, Fp32, 0, Fp32);
    check_family(20, 6, {128, 128}, PROMP_ACT_TANH, Split, 1, Fp32);               // k_wide<128, 2> under the FP32 switch
    check_family(20, 8, {128, 128}, PROMP_ACT_TANH, Split, 1, Fp32);
    check_family(127, 1, {128, 128}, PROMP_ACT_TANH, Split, 3, Fp32);
    check_family(50, 4, {100, 100}, PROMP_ACT_TANH, Split, 1, Fp32);               // padded to (128, 128)
    check_padding(11, 7, {48, 20}, {64, 32});
    check_padding(40, 3, {48, 20}, {64, 64});
    check_padding(50, 4, {100, 100}, {128, 128});
    // instances the launches are written for
    EXPECT(chain_ksteps(8) == 2 && chain_ksteps(9) == 5 && chain_ksteps(20) == 5 && chain_ksteps(21) == 8 && chain_ksteps(32) == 8, "chain_ksteps");
    EXPECT(wide_nob(32) == 2 && wide_nob(33) == 4 && wide_nob(64) == 4 && wide_nob(65) == 8 && wide_nob(128) == 8, "wide_nob");
    EXPECT(wb_nko(1) == 4 && wb_nko(2) == 7 && wb_nko(3) == 8, "wb_nko");
    // refusals carry the message promp_last_error() hands out
    check_refused(make_dims(20, 65, {64, 64}), "act_dim 65 unsupported (1..64)");
    check_refused(make_dims(1025, 6, {64, 64}), "obs_dim 1025 unsupported (1..1024)");
    check_refused(make_dims(20, 6, {64, 64, 64, 64, 64}), "hidden_sizes of length 5 unsupported (1..4 hidden layers)");
    check_refused(make_dims(20, 6, {64, 64}, 3), "hidden_act 3 unknown (0 tanh, 1 relu, 2 identity)");
    {
        promp_dims d = make_dims(20, 6, {64, 64});
        d.num_inner_steps = PROMP_ETA_MAX + 1;
        check_refused(d, "num_inner_steps must be in [1, 8]");
    }
    {
        std::string why;
        EXPECT(check_dims(nullptr, &why) == -1 && why == "dims is NULL", "check_dims(NULL): '%s'", why.c_str());
    }
    const promp_dims d = make_dims(20, 6, {64, 64});
    EXPECT(feature_dim(&d, PROMP_BASELINE_LINEAR_FEATURE) == 44 && feature_dim(&d, PROMP_BASELINE_LINEAR_TIME) == 4 && feature_dim(&d, PROMP_BASELINE_ZERO) == 0, "feature_dim");
}

// ---- step tables ---------------------------------------------------------------------------------------------------------
// offsets in exactly sized heap blocks (the sanitizer sees a read past either end)
struct Offsets {
    int M = 0, n_paths = 0;
    std::unique_ptr<int32_t[]> tpo, pro;
    Offsets(const std::vector<int>& t, const std::vector<int>& p) : M((int)t.size() - 1), n_paths((int)p.size() - 1), tpo(new int32_t[t.size()]), pro(new int32_t[p.size()]) {
        std::copy(t.begin(), t.end(), tpo.get());
        std::copy(p.begin(), p.end(), pro.get());
    }
};
static Offsets offsets_of(const std::vector<std::vector<int>>& lengths) {
    std::vector<int> t{0}, p{0};
    for (const auto& task : lengths) {
        for (int n : task) p.push_back(p.back() + n);
        t.push_back((int)p.size() - 1);
    }
    return Offsets(t, p);
}
static void check_tables(const char* name, const std::vector<std::vector<int>>& lengths, int n_cus) {
    const Offsets o = offsets_of(lengths);
    const int M = o.M, R = o.pro[o.n_paths], max_work = 2 * n_cus + M;
    StepTables T;
    std::string why;
    const int rc = build_step_tables(n_cus, max_work, R, o.n_paths, M, o.n_paths, o.tpo.get(), o.pro.get(), &T, &why);
    EXPECT(rc == 0, "%s at %d CUs: refused (%d): %s", name, n_cus, rc, why.c_str());
    if (rc) return;
#define TEXPECT(cond, ...) do { if (!(cond)) { EXPECT(cond, __VA_ARGS__); printf("    (%s at %d CUs)\n", name, n_cus); return; } } while (0)
    // offsets and time indices
    TEXPECT((int)T.pro.size() == o.n_paths + 1 && (int)T.tpo.size() == M + 1 && (int)T.tro.size() == M + 1 && (int)T.row_t.size() == R &&
            (int)T.path_task.size() == o.n_paths, "table sizes");
    for (int i = 0; i <= M; ++i) TEXPECT(T.tpo[i] == o.tpo[i] && T.tro[i] == o.pro[o.tpo[i]], "task %d: offsets", i);
    for (int i = 0; i < M; ++i)
        for (int p = o.tpo[i]; p < o.tpo[i + 1]; ++p) {
            TEXPECT(T.pro[p] == o.pro[p] && T.pro[p + 1] == o.pro[p + 1] && T.path_task[p] == i, "path %d: offsets / task", p);
            for (int r = o.pro[p]; r < o.pro[p + 1]; ++r) TEXPECT(T.row_t[r] == r - o.pro[p], "row %d of path %d: time index %d", r, p, T.row_t[r]);
        }
    // work tables
    for (int t = 0; t < 2; ++t) {
        const auto& W = T.work[t];
        const auto& off = T.two[t];
        TEXPECT((int)off.size() == M + 1 && off[0] == 0 && off[M] == (int)W.size(), "work table %d: task offsets do not span the list", t);
        TEXPECT((int)W.size() <= max_work, "work table %d: %zu items, room for %d", t, W.size(), max_work);
        for (int i = 0; i < M; ++i) {
            const int tiles = (T.tro[i + 1] - T.tro[i] + 15) / 16, n = off[i + 1] - off[i];
            TEXPECT(n >= 1 && n <= tiles, "work table %d: task %d has %d items for %d tiles", t, i, n, tiles);
            int row = T.tro[i];
            for (int k = off[i]; k < off[i + 1]; ++k) {
                TEXPECT(W[k].task == i && W[k].row_begin == row && W[k].row_end > W[k].row_begin && W[k].pad == 0, "work table %d item %d: task %d rows [%d, %d), expected task %d from row %d",
                        t, k, W[k].task, W[k].row_begin, W[k].row_end, i, row);
                TEXPECT((W[k].row_begin - T.tro[i]) % 16 == 0, "work table %d item %d: begins %d rows into its task", t, k, W[k].row_begin - T.tro[i]);
                row = W[k].row_end;
            }
            TEXPECT(row == T.tro[i + 1], "work table %d: task %d covered up to row %d of %d", t, i, row, T.tro[i + 1]);
        }
    }
    // chain segments
    const int nseg = (int)T.segs.size(), nwg = (int)T.wg_off.size() - 1;
    TEXPECT(nseg <= max_work, "%d segments, room for %d", nseg, max_work);
    TEXPECT((int)T.slot_chain.size() == M + 1 && T.slot_chain[0] == 0 && T.slot_chain[M] == nseg, "slot offsets do not span the segment list");
    for (int i = 0; i < M; ++i) {
        const int tiles = (T.tro[i + 1] - T.tro[i] + 15) / 16;
        TEXPECT(T.slot_chain[i + 1] > T.slot_chain[i], "task %d has no segment", i);
        int tile = 0;
        for (int k = T.slot_chain[i]; k < T.slot_chain[i + 1]; ++k) {
            const ChainSeg& s = T.segs[k];
            TEXPECT(s.task == i && s.tile0 == tile && s.ntiles > 0 && s.pad == 0, "segment %d: task %d tiles [%d, +%d), expected task %d from tile %d", k, s.task, s.tile0, s.ntiles, i, tile);
            TEXPECT(s.tile0 % 4 == 0, "segment %d: tile0 %d", k, s.tile0);
            tile += s.ntiles;
        }
        TEXPECT(tile == tiles, "task %d: segments cover %d of %d tiles", i, tile, tiles);
    }
    TEXPECT(nwg >= 1 && nwg <= n_cus, "%d workgroups on %d CUs", nwg, n_cus);
    TEXPECT(T.wg_off[0] == 0 && T.wg_off[nwg] == nseg, "workgroup offsets do not span the segment list");
    for (int g = 0; g < nwg; ++g) TEXPECT(T.wg_off[g + 1] > T.wg_off[g], "workgroup %d has no segment", g);
#undef TEXPECT
}
static void check_malformed(const char* name, int M, int n_paths, int max_rows, int max_paths, const std::vector<int>& t, const std::vector<int>& p, const char* want) {
    const Offsets o(t, p);
    StepTables T;
    std::string why;
    const int rc = build_step_tables(8, 16 + M, max_rows, max_paths, M, n_paths, o.tpo.get(), o.pro.get(), &T, &why);
    EXPECT(rc == -1 && why == want, "%s: returned %d '%s', expected -1 '%s'", name, rc, why.c_str(), want);
    EXPECT(T.row_t.empty() && T.segs.empty() && T.work[0].empty(), "%s: tables written on refusal", name);
}
// Table 0 of a layout at n_cus compute units must be exactly the row ranges `want` (pairs of begin, end), in order.
// tests/layered_checks.py relies on it: PROMP_MAX_CUS=1 makes every task ONE work item (so that the layer-by-layer kernels walk
// several rounds, chunks and loss blocks per item), PROMP_MAX_CUS=2 cuts a one-task batch of 513 rows at row 256.
static void check_long_items(const char* name, const std::vector<std::vector<int>>& lengths, int n_cus, const std::vector<std::pair<int, int>>& want) {
    const Offsets o = offsets_of(lengths);
    const int M = o.M, R = o.pro[o.n_paths];
    StepTables T;
    std::string why;
    const int rc = build_step_tables(n_cus, 2 * n_cus + M, R, o.n_paths, M, o.n_paths, o.tpo.get(), o.pro.get(), &T, &why);
    EXPECT(rc == 0, "%s at %d CUs: refused (%d): %s", name, n_cus, rc, why.c_str());
    if (rc) return;
    const auto& W = T.work[0];
    EXPECT(W.size() == want.size(), "%s at %d CUs: table 0 has %zu items, expected %zu", name, n_cus, W.size(), want.size());
    if (W.size() != want.size()) return;
    for (size_t k = 0; k < W.size(); ++k)
        EXPECT(W[k].row_begin == want[k].first && W[k].row_end == want[k].second, "%s at %d CUs: item %zu is rows [%d, %d), expected [%d, %d)", name, n_cus,
               k, W[k].row_begin, W[k].row_end, want[k].first, want[k].second);
}
// The chain kernels' segment list (task, tile0, ntiles) and the workgroups' offsets into it must be exactly `want` / `want_wg`.
// tests/fused_checks.py relies on it as on check_long_items: which of its row cases gives a wave several tiles, a workgroup
// several segments, a task two partial rows or a segment with tile0 > 0 is decided here.
struct Seg { int task, tile0, ntiles; };
static void check_chain_segments(const char* name, const std::vector<std::vector<int>>& lengths, int n_cus, const std::vector<Seg>& want,
                                 const std::vector<int>& want_wg) {
    const Offsets o = offsets_of(lengths);
    const int M = o.M, R = o.pro[o.n_paths];
    StepTables T;
    std::string why;
    const int rc = build_step_tables(n_cus, 2 * n_cus + M, R, o.n_paths, M, o.n_paths, o.tpo.get(), o.pro.get(), &T, &why);
    EXPECT(rc == 0, "%s at %d CUs: refused (%d): %s", name, n_cus, rc, why.c_str());
    if (rc) return;
    EXPECT(T.segs.size() == want.size(), "%s at %d CUs: %zu segments, expected %zu", name, n_cus, T.segs.size(), want.size());
    if (T.segs.size() != want.size()) return;
    for (size_t k = 0; k < want.size(); ++k)
        EXPECT(T.segs[k].task == want[k].task && T.segs[k].tile0 == want[k].tile0 && T.segs[k].ntiles == want[k].ntiles,
               "%s at %d CUs: segment %zu is task %d tiles [%d, +%d), expected task %d tiles [%d, +%d)", name, n_cus, k, T.segs[k].task,
               T.segs[k].tile0, T.segs[k].ntiles, want[k].task, want[k].tile0, want[k].ntiles);
    EXPECT(T.wg_off == want_wg, "%s at %d CUs: the workgroups' segment offsets differ (%zu workgroups, expected %zu)", name, n_cus,
           T.wg_off.size() - 1, want_wg.size() - 1);
    // a task's partial rows are its segments
    int slot = 0;
    for (int i = 0; i < M; ++i) {
        int n = 0;
        for (const Seg& s : want) n += s.task == i;
        EXPECT(T.slot_chain[i] == slot && T.slot_chain[i + 1] == slot + n, "%s at %d CUs: task %d has partial rows [%d, %d), expected [%d, %d)", name, n_cus,
               i, T.slot_chain[i], T.slot_chain[i + 1], slot, slot + n);
        slot += n;
    }
}
// the row cases of tests/fused_checks.py (ROW_CASES A-E, DICE_LENGTHS, the split-range batch): work table 0 and the segment table
static void check_fused_row_cases() {
    const std::vector<std::vector<int>> A{{16}, {17}, {64, 1}, {80}}, B{{200, 55}, {256}, {256, 1}}, C{{300, 21}, {1}, {130}},
        D{{100}, {100}, {100}}, E{{513}}, dice{{256, 65}, {64, 1, 129}}, range{{160, 160}, {160, 160}};
    // A: waves without a tile (1, 2 tiles on four waves), a second tile of one row (65 rows); a third 32-row round of one row and a
    //    second 64-row round of one row on the cooperative kernels
    check_long_items("fused rows A", A, 1, {{0, 16}, {16, 33}, {33, 98}, {98, 178}});
    check_chain_segments("fused rows A", A, 1, {{0, 0, 1}, {1, 0, 2}, {2, 0, 5}, {3, 0, 5}}, {0, 4});
    // B: four and five tiles per wave; 3 rounds of 64 + 63 rows, exactly 4, 4 + 1 row
    check_long_items("fused rows B", B, 1, {{0, 255}, {255, 511}, {511, 768}});
    check_chain_segments("fused rows B", B, 1, {{0, 0, 16}, {1, 0, 16}, {2, 0, 17}}, {0, 3});
    // C: a one-row task between a 21-tile and a 9-tile one
    check_long_items("fused rows C", C, 1, {{0, 321}, {321, 322}, {322, 452}});
    check_chain_segments("fused rows C", C, 1, {{0, 0, 21}, {1, 0, 1}, {2, 0, 9}}, {0, 3});
    // D: the middle task split between the two workgroups at tile 4 (two partial rows, a segment with tile0 != 0)
    check_long_items("fused rows D", D, 2, {{0, 100}, {100, 200}, {200, 300}});
    check_chain_segments("fused rows D", D, 2, {{0, 0, 7}, {1, 0, 4}, {1, 4, 3}, {2, 0, 7}}, {0, 2, 4});
    // E: tile0 = 20; cooperative items that begin 256 rows into the task
    check_long_items("fused rows E", E, 2, {{0, 256}, {256, 513}});
    check_chain_segments("fused rows E", E, 2, {{0, 0, 20}, {0, 20, 13}}, {0, 1, 2});
    check_long_items("fused dice lengths", dice, 1, {{0, 321}, {321, 515}});
    check_chain_segments("fused dice lengths", dice, 1, {{0, 0, 21}, {1, 0, 13}}, {0, 2});
    // check_split_range at M = 2, P = 2, T = 160 on one unit: one workgroup walks two 20-tile segments
    check_long_items("fused split range", range, 1, {{0, 320}, {320, 640}});
    check_chain_segments("fused split range", range, 1, {{0, 0, 20}, {1, 0, 20}}, {0, 2});
}
// More tasks than compute units (tests/count_axis_checks.py: M = n_cus + 1): 257 one-tile tasks on 256 units.  Every task is floored
// to one work item in both tables -- 257 items each, nothing left to share out, room for max_work = 2 * 256 + 257 = 769 --, and there
// are 257 chain segments of one tile.  A workgroup of one segment costs 6 quarter rounds; 257 of them are one too many, and the
// smallest cost limit that admits a second segment (12) pairs them up: 128 workgroups of two tasks and one of the last task alone,
// every workgroup but the last changing task mid-launch.
static void check_more_tasks_than_units() {
    const int M = 257, n_cus = 256;
    const std::vector<std::vector<int>> lengths(M, std::vector<int>{16});
    std::vector<std::pair<int, int>> items;
    std::vector<Seg> segs;
    std::vector<int> wg{0};
    for (int i = 0; i < M; ++i) {
        items.push_back({16 * i, 16 * i + 16});
        segs.push_back({i, 0, 1});
        if (i % 2 == 1 || i == M - 1) wg.push_back(i + 1);
    }
    check_long_items("257 one-tile tasks", lengths, n_cus, items);
    check_chain_segments("257 one-tile tasks", lengths, n_cus, segs, wg);
    EXPECT(wg.size() == 130, "257 one-tile tasks: %zu workgroups expected by the test itself", wg.size() - 1);
    const Offsets o = offsets_of(lengths);
    StepTables T;
    std::string why;
    const int rc = build_step_tables(n_cus, 2 * n_cus + M, 16 * M, M, M, M, o.tpo.get(), o.pro.get(), &T, &why);
    EXPECT(rc == 0 && T.work[1].size() == (size_t)M, "257 one-tile tasks: table 1 has %zu items (%d): %s", T.work[1].size(), rc, why.c_str());
    for (int i = 0; rc == 0 && i < M && i < (int)T.work[1].size(); ++i)
        EXPECT(T.work[1][i].task == i && T.work[1][i].row_begin == 16 * i && T.work[1][i].row_end == 16 * i + 16, "257 one-tile tasks: table 1 item %d", i);
    // the same tasks with a room one short of the items are refused by name, nothing written
    StepTables S;
    const int rc2 = build_step_tables(n_cus, M - 1, 16 * M, M, M, M, o.tpo.get(), o.pro.get(), &S, &why);
    EXPECT(rc2 == -5 && why == "internal: work table overflow (257 > 256)" && S.segs.empty(), "257 one-tile tasks, room for 256: returned %d '%s'", rc2, why.c_str());
}
static void check_step_tables() {
    check_fused_row_cases();
    check_more_tasks_than_units();
    // one compute unit: one item per task, whatever the row counts (the work-item lengths of tests/layered_checks.py)
    check_long_items("one task, one item", {{300, 21}}, 1, {{0, 321}});
    check_long_items("three ragged tasks, one item each", {{300, 21}, {256, 256, 1}, {1}}, 1, {{0, 321}, {321, 834}, {834, 835}});
    check_long_items("three ragged tasks, one item each", {{16}, {17}, {32, 1}}, 1, {{0, 16}, {16, 33}, {33, 66}});
    check_long_items("three ragged tasks, one item each", {{200, 55}, {256}, {256, 1}}, 1, {{0, 255}, {255, 511}, {511, 768}});
    // two compute units, one task of 513 rows (33 tiles): two items that meet at row 256
    check_long_items("513 rows on two units", {{513}}, 2, {{0, 256}, {256, 513}});
    const std::vector<int> edge{1, 2, 63, 64, 65, 127, 128, 129};        // around the scans' 64-row chunks (EDGE_LENGTHS)
    for (int n_cus : {2, 8, 256}) {
        check_tables("one row", {{1}}, n_cus);
        check_tables("ragged", {{3}, std::vector<int>(20, 200), {64, 64}}, n_cus);
        check_tables("chunk edges", {edge}, n_cus);
        check_tables("chunk edges, two tasks", {edge, {1}}, n_cus);
        check_tables("40 x 20 x 200", std::vector<std::vector<int>>(40, std::vector<int>(20, 200)), n_cus);
        check_tables("300 tasks of 17 rows", std::vector<std::vector<int>>(300, std::vector<int>{17}), n_cus);
    }
    check_malformed("task offsets start at 1", 2, 3, 100, 10, {1, 2, 3}, {0, 5, 10, 15}, "task_path_offsets must start at 0 and end at n_paths");
    check_malformed("task offsets end early", 2, 3, 100, 10, {0, 1, 2}, {0, 5, 10, 15}, "task_path_offsets must start at 0 and end at n_paths");
    check_malformed("row offsets start at 1", 2, 3, 100, 10, {0, 1, 3}, {1, 5, 10, 15}, "path_row_offsets must start at 0");
    check_malformed("row offsets decrease", 1, 2, 100, 10, {0, 2}, {0, 50, 10}, "path_row_offsets must be non-decreasing");
    check_malformed("row offsets decrease in a later task", 2, 3, 100, 10, {0, 1, 3}, {0, 5, 90, 15}, "path_row_offsets must be non-decreasing");
    check_malformed("task offsets decrease", 2, 3, 100, 10, {0, 5, 3}, {0, 5, 10, 15}, "task 1 has no paths");
    check_malformed("task without paths", 2, 2, 100, 10, {0, 0, 2}, {0, 5, 10}, "task 0 has no paths");
    check_malformed("task without rows", 2, 2, 100, 10, {0, 1, 2}, {0, 0, 5}, "task 0 has no rows");
    check_malformed("last task without rows", 2, 3, 100, 10, {0, 1, 3}, {0, 5, 5, 5}, "task 1 has no rows");
    check_malformed("too many rows", 1, 1, 100, 10, {0, 1}, {0, 101}, "rows 101 outside [1, max_rows=100]");
    check_malformed("no rows at all", 1, 1, 100, 10, {0, 1}, {0, 0}, "rows 0 outside [1, max_rows=100]");
    check_malformed("too many paths", 1, 11, 100, 10, {0, 11}, std::vector<int>(12, 0), "n_paths 11 outside [1, max_paths=10]");
    check_malformed("no paths", 1, 0, 100, 10, {0, 0}, {0}, "n_paths 0 outside [1, max_paths=10]");
}

// ---- k_gram_tiled's wave -> square map -----------------------------------------------------------------------------------------
static void check_gramt(int nblk) {
    const int NWV = GRAMT_NWV, TB = GRAMT_TB, nb = (nblk + TB - 1) / TB, nr = nb * (nb + 1) / 2;
    EXPECT(gramt_nb(nblk) == nb && gramt_nrect(nblk) == nr, "nblk %d: %d bands, %d squares", nblk, gramt_nb(nblk), gramt_nrect(nblk));
    GramtMap map;
    memset(&map, 7, sizeof map);
    gramt_balance(nblk, NWV, &map);
    if (nr > NWV) {      // slices in list order: the kernel ignores the map
        for (int w = 0; w < 16; ++w) EXPECT(map.rect[w] == 255 && map.part[w] == GRAMT_DIAG, "nblk %d: wave %d mapped (%d, %d) with %d squares", nblk, w, map.rect[w], map.part[w], nr);
        return;
    }
    std::vector<int> diag(nr, 0);
    for (int bi = 0, r = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj, ++r) diag[r] = bi == bj;
    std::vector<int> whole(nr, 0), top(nr, 0), rest(nr, 0);
    int load[4] = {0, 0, 0, 0}, count[4] = {0, 0, 0, 0};
    for (int w = 0; w < NWV; ++w) {
        const int r = map.rect[w], part = map.part[w];
        if (r == 255) continue;
        EXPECT(r < nr, "nblk %d: wave %d takes square %d of %d", nblk, w, r, nr);
        if (r >= nr) return;
        int cost = 0;
        if (part == GRAMT_FULL) { EXPECT(!diag[r], "nblk %d: diagonal square %d issued whole", nblk, r); whole[r]++; cost = TB * TB; }
        else if (part == GRAMT_DIAG) { EXPECT(diag[r], "nblk %d: square %d issued as a triangle", nblk, r); whole[r]++; cost = TB * (TB + 1) / 2; }
        else if (part == GRAMT_DIAG_TOP) { EXPECT(diag[r], "nblk %d: square %d split", nblk, r); top[r]++; cost = TB; }
        else if (part == GRAMT_DIAG_REST) { EXPECT(diag[r], "nblk %d: square %d split", nblk, r); rest[r]++; cost = TB * (TB + 1) / 2 - TB; }
        else EXPECT(false, "nblk %d: wave %d has part %d", nblk, w, part);
        load[w & 3] += cost;
        count[w & 3]++;
    }
    for (int r = 0; r < nr; ++r)
        EXPECT((whole[r] == 1 && top[r] == 0 && rest[r] == 0) || (whole[r] == 0 && top[r] == 1 && rest[r] == 1),
               "nblk %d: square %d appears %d times whole, %d / %d times in halves", nblk, r, whole[r], top[r], rest[r]);
    // wave w runs on SIMD w mod 4: the four carry the same pieces up to one (by count, and by products up to the largest piece)
    const int lmax = *std::max_element(load, load + 4), lmin = *std::min_element(load, load + 4);
    const int cmax = *std::max_element(count, count + 4), cmin = *std::min_element(count, count + 4);
    EXPECT(cmax - cmin <= 1, "nblk %d: %d .. %d pieces per SIMD", nblk, cmin, cmax);
    EXPECT(lmax - lmin <= TB * TB, "nblk %d: %d .. %d products per SIMD", nblk, lmin, lmax);
    EXPECT(std::accumulate(load, load + 4, 0) == (nr - nb) * TB * TB + nb * TB * (TB + 1) / 2, "nblk %d: %d products in all", nblk, std::accumulate(load, load + 4, 0));
}

int main() {
    check_dispatch();
    check_shapes();
    check_step_tables();
    for (int nblk : {13, 15, 18, 48}) check_gramt(nblk);
    if (g_failed) printf("%d expectation(s) failed\n", g_failed);
    else printf("plan_check: all expectations hold\n");
    return g_failed ? 1 : 0;
}
