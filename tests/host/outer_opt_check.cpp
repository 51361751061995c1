// outer_opt_check.cpp -- the outer step's planning of promp_amd/csrc/promp_plan.h, checked on the host alone.
//
// Stand-alone: includes the plan header and nothing else of the project.  tests/test_outer_optimizer_host.py compiles it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined
// and runs it once.  One line per failed expectation, exit status 1 if there was any.
//
//   names        outer_rule_by_name / outer_rule_name: the three rules under their short names and TF1's class names, nothing else
//   validation   outer_opt_plan refuses with its message and writes nothing; only the arguments of the rule asked for are read
//   constants    default arguments give the plain kernels' 0.9f / 0.1f / 0.999f / 0.001f / 1e-8f and their lr_t, bit for bit
//   family       final_stage_plan: default settings give the plain instances; anything else, or the switch, the general family on
//                stepping evaluations only; the clip gives the split route
//   grids        final_stage_launch: the exchange buffer's floats and the grids of the reduce, mean and fused launches at the sizes
//                where a column block, a thread block or the statistics thread sits on an edge, against literals
#include "../../promp_amd/csrc/promp_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

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

static void check_names() {
    const struct { const char* name; int rule; } rows[] = {
        {"adam", PROMP_OUTER_ADAM}, {"AdamOptimizer", PROMP_OUTER_ADAM},
        {"sgd", PROMP_OUTER_SGD}, {"gradient_descent", PROMP_OUTER_SGD}, {"GradientDescentOptimizer", PROMP_OUTER_SGD},
        {"momentum", PROMP_OUTER_MOMENTUM}, {"MomentumOptimizer", PROMP_OUTER_MOMENTUM},
        {"rmsprop", -1}, {"RMSPropOptimizer", -1}, {"Adam", -1}, {"", -1}, {"adagrad", -1},
    };
    for (const auto& r : rows) EXPECT(outer_rule_by_name(r.name) == r.rule, "'%s' -> %d", r.name, outer_rule_by_name(r.name));
    EXPECT(outer_rule_by_name(nullptr) == -1, "NULL name");
    for (int rule = 0; rule < 3; ++rule) EXPECT(outer_rule_by_name(outer_rule_name(rule)) == rule, "rule %d", rule);
    EXPECT(outer_rule_name(3) == nullptr && outer_rule_name(-1) == nullptr, "names of unknown rules");
}

static bool same_plan(const OuterOptPlan& a, const OuterOptPlan& b) {
    return a.rule == b.rule && a.b1 == b.b1 && a.b2 == b.b2 && a.eps == b.eps && a.mu == b.mu && a.nesterov == b.nesterov && a.max_norm == b.max_norm;
}

static void check_validation() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    OuterOptPlan sentinel;
    sentinel.rule = PROMP_OUTER_MOMENTUM; sentinel.mu = 0.25f; sentinel.max_norm = 3.f;
    auto refused = [&](int rule, const float* args, float c, const char* needle) {
        OuterOptPlan p = sentinel;
        std::string why;
        const int rc = outer_opt_plan(rule, args, c, &p, &why);
        EXPECT(rc == -1, "rule %d accepted (%s)", rule, needle);
        EXPECT(why.find(needle) != std::string::npos, "message '%s' lacks '%s'", why.c_str(), needle);
        EXPECT(same_plan(p, sentinel), "a refused plan was written (%s)", needle);
    };
    const float good[4] = {0.9f, 0.999f, 1e-8f, 0.f};
    refused(3, good, 0.f, "rule 3 unknown");
    refused(-1, nullptr, 0.f, "rule -1 unknown");
    refused(PROMP_OUTER_SGD, nullptr, -1.f, "max_grad_norm");
    refused(PROMP_OUTER_SGD, nullptr, inf, "max_grad_norm");
    refused(PROMP_OUTER_SGD, nullptr, nan, "max_grad_norm");
    { const float a[4] = {1.f, 0.999f, 1e-8f, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "beta1"); }
    { const float a[4] = {-0.1f, 0.999f, 1e-8f, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "beta1"); }
    { const float a[4] = {nan, 0.999f, 1e-8f, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "beta1"); }
    { const float a[4] = {0.9f, 1.f, 1e-8f, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "beta2"); }
    { const float a[4] = {0.9f, 0.999f, 0.f, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "epsilon"); }
    { const float a[4] = {0.9f, 0.999f, -1e-8f, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "epsilon"); }
    { const float a[4] = {0.9f, 0.999f, inf, 0.f}; refused(PROMP_OUTER_ADAM, a, 0.f, "epsilon"); }
    { const float a[4] = {1.f, 0.f, 0.f, 0.f}; refused(PROMP_OUTER_MOMENTUM, a, 0.f, "momentum"); }
    { const float a[4] = {0.5f, 2.f, 0.f, 0.f}; refused(PROMP_OUTER_MOMENTUM, a, 0.f, "use_nesterov"); }
    // only the arguments of the rule asked for are read: SGD takes anything
    {
        const float junk[4] = {7.f, -3.f, nan, inf};
        OuterOptPlan p;
        std::string why;
        EXPECT(outer_opt_plan(PROMP_OUTER_SGD, junk, 0.5f, &p, &why) == 0, "SGD refused: %s", why.c_str());
        EXPECT(p.rule == PROMP_OUTER_SGD && p.max_norm == 0.5f, "SGD plan");
    }
    // round trip through promp_get_outer_optimizer's layout
    {
        const float a[4] = {0.5f, 1.f, 0.f, 0.f};
        OuterOptPlan p;
        std::string why;
        EXPECT(outer_opt_plan(PROMP_OUTER_MOMENTUM, a, 2.f, &p, &why) == 0, "momentum refused: %s", why.c_str());
        int rule = -1;
        float out[4] = {9.f, 9.f, 9.f, 9.f}, c = -1.f;
        outer_opt_unplan(p, &rule, out, &c);
        EXPECT(rule == PROMP_OUTER_MOMENTUM && out[0] == 0.5f && out[1] == 1.f && out[2] == 0.f && out[3] == 0.f && c == 2.f, "unplan");
        outer_opt_unplan(p, nullptr, nullptr, nullptr);
        const OuterOptArgs o = outer_opt_args(p);
        EXPECT(o.rule == PROMP_OUTER_MOMENTUM && o.mu == 0.5f && o.nesterov == 1 && o.max_norm == 2.f, "args of momentum");
        EXPECT(outer_lr_t(p, 0.25f, 1) == 0.25f && outer_lr_t(p, 0.25f, 1000) == 0.25f, "momentum: lr as given");
    }
}

static void check_constants() {
    const OuterOptPlan def;
    EXPECT(outer_opt_is_default(def), "a fresh plan is the default");
    // asking for the defaults by value is the default: the float32 values mean the double constants
    const float a[4] = {0.9f, 0.999f, 1e-8f, 0.f};
    OuterOptPlan p;
    std::string why;
    EXPECT(outer_opt_plan(PROMP_OUTER_ADAM, a, 0.f, &p, &why) == 0 && outer_opt_is_default(p) && same_plan(p, def), "defaults by value");
    EXPECT(outer_opt_plan(PROMP_OUTER_ADAM, nullptr, 0.f, &p, &why) == 0 && outer_opt_is_default(p), "defaults by NULL");
    const OuterOptArgs o = outer_opt_args(def);
    EXPECT(o.b1 == 0.9f && o.one_minus_b1 == 0.1f && o.b2 == 0.999f && o.one_minus_b2 == 0.001f && o.eps == 1e-8f && o.max_norm == 0.f,
           "%.9g %.9g %.9g %.9g %.9g", o.b1, o.one_minus_b1, o.b2, o.one_minus_b2, o.eps);
    // lr_t: the line promp_adam_step always had
    for (long long t : {1LL, 2LL, 5LL, 100LL, 100000LL})
        for (float lr : {1e-3f, 0.5f}) {
            const double td = (double)t;
            const float was = (float)((double)lr * std::sqrt(1.0 - std::pow(0.999, td)) / (1.0 - std::pow(0.9, td)));
            EXPECT(outer_lr_t(def, lr, t) == was, "t %lld lr %g: %.9g vs %.9g", t, lr, outer_lr_t(def, lr, t), was);
        }
    // other arguments: the differences are rounded from the double difference of the float32 value
    const float b[4] = {0.8f, 0.99f, 1e-5f, 0.f};
    EXPECT(outer_opt_plan(PROMP_OUTER_ADAM, b, 0.f, &p, &why) == 0 && !outer_opt_is_default(p), "other arguments");
    const OuterOptArgs q = outer_opt_args(p);
    EXPECT(q.b1 == 0.8f && q.one_minus_b1 == (float)(1.0 - (double)0.8f) && q.b2 == 0.99f && q.one_minus_b2 == (float)(1.0 - (double)0.99f) && q.eps == 1e-5f,
           "arguments of Adam(0.8, 0.99, 1e-5)");
    EXPECT(outer_lr_t(p, 1e-3f, 3) == (float)(1e-3f * std::sqrt(1.0 - std::pow((double)0.99f, 3.0)) / (1.0 - std::pow((double)0.8f, 3.0))), "lr_t of other betas");
}

static void check_family() {
    const PlanSwitches off;
    PlanSwitches forced;
    forced.outer_generic = true;
    const OuterOptPlan def;
    for (int stepping = 0; stepping < 2; ++stepping)
        for (int split = 0; split < 2; ++split) {
            const FinalPlan f = final_stage_plan(def, off, stepping, split);
            EXPECT(!f.general && f.split == (split != 0), "default settings: the plain instances, the route the ranks ask for");
            const FinalPlan g = final_stage_plan(def, forced, stepping, split);
            EXPECT(g.general == (stepping != 0) && g.split == (split != 0), "the switch: general where a step is taken, same route");
        }
    struct { int rule; float args[4]; float c; } others[] = {
        {PROMP_OUTER_ADAM, {0.9f, 0.999f, 1e-5f, 0.f}, 0.f}, {PROMP_OUTER_ADAM, {0.8f, 0.999f, 1e-8f, 0.f}, 0.f},
        {PROMP_OUTER_ADAM, {0.9f, 0.99f, 1e-8f, 0.f}, 0.f},  {PROMP_OUTER_SGD, {0.f, 0.f, 0.f, 0.f}, 0.f},
        {PROMP_OUTER_MOMENTUM, {0.f, 0.f, 0.f, 0.f}, 0.f},   {PROMP_OUTER_ADAM, {0.9f, 0.999f, 1e-8f, 0.f}, 1.f},
        {PROMP_OUTER_SGD, {0.f, 0.f, 0.f, 0.f}, 0.5f},
    };
    for (const auto& o : others) {
        OuterOptPlan p;
        std::string why;
        EXPECT(outer_opt_plan(o.rule, o.args, o.c, &p, &why) == 0, "refused: %s", why.c_str());
        EXPECT(!outer_opt_is_default(p), "rule %d is not the default", o.rule);
        for (int split = 0; split < 2; ++split) {
            const FinalPlan f = final_stage_plan(p, off, true, split);
            EXPECT(f.general, "rule %d clip %g: the general family", o.rule, o.c);
            EXPECT(f.split == (split != 0 || o.c > 0.f), "rule %d clip %g: the clip takes the split route", o.rule, o.c);
            const FinalPlan e = final_stage_plan(p, off, false, split);
            EXPECT(!e.general && e.split == (split != 0), "an evaluation that does not step stays on the plain instances");
        }
    }
}

static void check_grids() {
    // Theta, K, step sizes trained, floats of the exchange buffer, blocks of the reduce / mean / fused launch
    const struct { int NP, K; bool sizes; size_t red; unsigned reduce, mean, fused; } rows[] = {
        {60, 1, false, 63, 1, 1, 2},           {60, 1, true, 123, 2, 1, 3},           {60, 2, false, 64, 1, 1, 2},
        {60, 2, true, 124, 2, 1, 3},           {62, 1, false, 65, 2, 1, 3},           {62, 1, true, 127, 2, 1, 3},
        {62, 2, false, 66, 2, 1, 3},           {62, 2, true, 128, 2, 1, 3},           {255, 1, false, 258, 5, 1, 6},
        {255, 1, true, 513, 9, 2, 10},         {255, 2, false, 259, 5, 1, 6},         {255, 2, true, 514, 9, 2, 10},
        {256, 1, false, 259, 5, 2, 6},         {256, 1, true, 515, 9, 3, 10},         {256, 2, false, 260, 5, 2, 6},
        {256, 2, true, 516, 9, 3, 10},         {5900, 1, false, 5903, 93, 24, 94},    {5900, 1, true, 11803, 185, 47, 186},
        {5900, 2, false, 5904, 93, 24, 94},    {5900, 2, true, 11804, 185, 47, 186},  {31888, 1, false, 31891, 499, 125, 500},
        {31888, 1, true, 63779, 997, 250, 998}, {31888, 2, false, 31892, 499, 125, 500}, {31888, 2, true, 63780, 997, 250, 998},
    };
    int n = 0;
    for (const auto& r : rows)
        for (int general = 0; general < 2; ++general)
            for (int split = 0; split < 2; ++split) {
                FinalPlan f;
                f.general = general != 0; f.split = split != 0;
                const FinalLaunch L = final_stage_launch(f, r.NP, r.K, r.sizes);
                EXPECT(L.general == f.general && L.split == f.split && L.sizes == r.sizes, "Theta %d: the plan is passed on", r.NP);
                EXPECT(L.red_count == r.red && final_red_count(r.NP, r.K, r.sizes) == r.red, "Theta %d K %d sizes %d: %zu floats, not %zu",
                       r.NP, r.K, (int)r.sizes, L.red_count, r.red);
                EXPECT(L.reduce_grid == r.reduce && L.mean_grid == r.mean && L.fused_grid == r.fused,
                       "Theta %d K %d sizes %d: grids %u %u %u, not %u %u %u", r.NP, r.K, (int)r.sizes, L.reduce_grid, L.mean_grid,
                       L.fused_grid, r.reduce, r.mean, r.fused);
                // 64 columns per reduce block: the last block holds a valid column, and no valid column is outside the grid
                EXPECT((size_t)(L.reduce_grid - 1) * 64 < L.red_count, "Theta %d: the last reduce block is empty", r.NP);
                EXPECT((size_t)L.reduce_grid * 64 >= L.red_count, "Theta %d: columns outside the reduce grid", r.NP);
                EXPECT(L.fused_grid == L.reduce_grid + 1, "Theta %d: the fused grid is the reduce grid and the statistics block", r.NP);
                // 256 threads per mean block: exactly the blocks of Theta + 1 (2 Theta + 1) threads
                const size_t threads = (size_t)(r.sizes ? 2 : 1) * r.NP + 1;
                EXPECT((size_t)L.mean_grid * 256 >= threads && (size_t)(L.mean_grid - 1) * 256 < threads, "Theta %d: mean grid %u for %zu threads",
                       r.NP, L.mean_grid, threads);
                ++n;
            }
    EXPECT(n == 6 * 2 * 2 * 4, "%d rows", n);
}

static void check_env() {
    unsetenv("PROMP_OUTER_GENERIC");
    EXPECT(!plan_switches_from_env().outer_generic, "unset");
    setenv("PROMP_OUTER_GENERIC", "1", 1);
    EXPECT(plan_switches_from_env().outer_generic, "=1");
    setenv("PROMP_OUTER_GENERIC", "0", 1);
    EXPECT(!plan_switches_from_env().outer_generic, "=0");
    unsetenv("PROMP_OUTER_GENERIC");
}

int main() {
    check_names();
    check_validation();
    check_constants();
    check_family();
    check_grids();
    check_env();
    if (g_failed) {
        printf("%d expectation(s) failed\n", g_failed);
        return 1;
    }
    printf("all expectations hold\n");
    return 0;
}
