// selection_check.cpp -- the selections of promp_amd/csrc/promp_plan.h (subsampled constraint products), checked on the host alone.
//
// Stand-alone: includes the plan header and nothing else of the project.  tests/test_selection_host.py compiles it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined
// and runs it once.  One line per failed expectation, exit status 1 if there was any.
//
//   counts       selection_count against exact integer arithmetic, at the factors and path counts where floor(f * P) in binary
//                floating point lands below the whole number (0.29 * 100)
//   refusals     unsorted, repeated, out of range, a task left with no path, negative n_sel: each with its message, and nothing
//                written (under the sanitizer: without a stray access either)
//   layout       the compact slab's offsets for a ragged three-task batch, and the step tables built on them
#include "../../promp_amd/csrc/promp_plan.h"

#include <cstdio>
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

static void check_counts() {
    const int pct[] = {10, 20, 25, 29, 30, 50, 70, 100};
    const int paths[] = {1, 3, 5, 10, 20, 100};
    for (int f : pct)
        for (int P : paths) {
            const int exact = f * P / 100 < 1 ? 1 : f * P / 100;
            const int got = selection_count(f / 100.0, P);
            EXPECT(got == exact, "f = %d%%, P = %d: %d paths, exact %d", f, P, got, exact);
            EXPECT(got >= 1 && got <= P, "f = %d%%, P = %d: %d paths", f, P, got);
        }
    EXPECT(selection_count(0.29, 100) == 29, "%d", selection_count(0.29, 100));
    EXPECT((int)(0.29 * 100) == 28, "the case the guard is there for no longer shows on this host");
}

// the ragged batch of tests/subsample_checks.py: 3 tasks with 5, 3 and 4 paths
static const int LEN[12] = {17, 16, 31, 1, 33, 9, 35, 18, 20, 3, 47, 15};
static const int32_t TPO[4] = {0, 5, 8, 12};

static void refuse(const std::vector<int32_t>& idx, int n_sel, const char* msg, const std::vector<int32_t>& pro) {
    SelectionLayout lay;
    lay.idx = {-7};
    std::string why;
    const int rc = build_selection(3, 12, TPO, pro.data(), n_sel, idx.empty() ? nullptr : idx.data(), &lay, &why);
    EXPECT(rc == -1, "rc %d for a selection that should be refused (%s)", rc, msg);
    EXPECT(why.find(msg) != std::string::npos, "message '%s' does not say '%s'", why.c_str(), msg);
    EXPECT(lay.idx.size() == 1 && lay.idx[0] == -7 && lay.tpo.empty() && lay.pro.empty(), "a refused selection wrote its output (%s)", msg);
}

static void check_layout() {
    std::vector<int32_t> pro(13, 0);
    for (int p = 0; p < 12; ++p) pro[p + 1] = pro[p] + LEN[p];
    refuse({1, 4, 3, 6, 9, 10}, 6, "not sorted", pro);
    refuse({1, 3, 3, 6, 9, 10}, 6, "repeats path 3", pro);
    refuse({1, 3, 6, 9, 12}, 5, "path index 12 out of range [0, 12)", pro);
    refuse({-1, 3, 6, 9}, 4, "path index -1 out of range", pro);
    refuse({0, 1, 2, 3, 4, 8, 9, 10, 11}, 9, "leaves task 1 with no path", pro);
    refuse({0, 5}, 2, "leaves task 2 with no path", pro);
    refuse({5, 8}, 2, "leaves task 0 with no path", pro);
    refuse({1, 3}, -1, "n_sel -1 is negative", pro);
    refuse({}, 0, "empty selection", pro);
    refuse({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11}, 13, "selection of 13 paths from a step of 12", pro);
    // one path left in task 1; the first path of tasks 0 and 2 dropped; the last path of the last task dropped
    const std::vector<std::vector<int32_t>> sels = {{1, 3, 4, 6, 9, 10}, {0, 2, 5, 7, 8, 10}, {1, 2, 3, 4, 5, 6, 7, 9, 10},
                                                    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
    for (const auto& sel : sels) {
        SelectionLayout lay;
        std::string why;
        const int n = (int)sel.size();
        const int rc = build_selection(3, 12, TPO, pro.data(), n, sel.data(), &lay, &why);
        EXPECT(rc == 0, "refused: %s", why.c_str());
        if (rc) continue;
        EXPECT(lay.idx == sel, "indices not kept");
        EXPECT((int)lay.tpo.size() == 4 && (int)lay.pro.size() == n + 1 && lay.tpo[0] == 0 && lay.tpo[3] == n && lay.pro[0] == 0, "offsets' ends");
        int rows = 0;
        for (int j = 0; j < n; ++j) {
            EXPECT(lay.pro[j + 1] - lay.pro[j] == LEN[sel[j]], "selected path %d has %d rows, path %d has %d", j, lay.pro[j + 1] - lay.pro[j], sel[j], LEN[sel[j]]);
            rows += LEN[sel[j]];
        }
        EXPECT(lay.pro[n] == rows, "%d rows, the selected paths hold %d", lay.pro[n], rows);
        for (int i = 0; i < 3; ++i) {
            int want = 0;
            for (int j = 0; j < n; ++j) want += sel[j] >= TPO[i] && sel[j] < TPO[i + 1];
            EXPECT(lay.tpo[i + 1] - lay.tpo[i] == want, "task %d keeps %d paths, selected %d", i, lay.tpo[i + 1] - lay.tpo[i], want);
            for (int j = lay.tpo[i]; j < lay.tpo[i + 1]; ++j) EXPECT(sel[j] >= TPO[i] && sel[j] < TPO[i + 1], "selected path %d filed under task %d", sel[j], i);
        }
        // the tables of the compact slab are those of an upload of the selected paths alone, sized by the selection
        for (int n_cus : {2, 256}) {
            StepTables t;
            const int trc = build_step_tables(n_cus, 2 * n_cus + 3, rows, n, 3, n, lay.tpo.data(), lay.pro.data(), &t, &why);
            EXPECT(trc == 0, "tables refused: %s", why.c_str());
            if (trc) continue;
            EXPECT((int)t.row_t.size() == rows && t.tro[3] == rows && t.tro[0] == 0, "rows of the tables");
            for (int i = 0; i < 3; ++i) EXPECT(t.tro[i] == lay.pro[lay.tpo[i]], "task %d starts at row %d", i, t.tro[i]);
            int covered = 0;
            for (const WorkItem& w : t.work[0]) {
                EXPECT(w.row_begin >= t.tro[w.task] && w.row_end <= t.tro[w.task + 1] && w.row_begin < w.row_end, "work item outside its task");
                covered += w.row_end - w.row_begin;
            }
            EXPECT(covered == rows, "work table 0 covers %d of %d rows", covered, rows);
            int tiles = 0, want_tiles = 0;
            for (const ChainSeg& s : t.segs) tiles += s.ntiles;
            for (int i = 0; i < 3; ++i) want_tiles += (t.tro[i + 1] - t.tro[i] + 15) / 16;
            EXPECT(tiles == want_tiles, "segments cover %d of %d tiles", tiles, want_tiles);
        }
    }
}

int main() {
    check_counts();
    check_layout();
    if (g_failed) printf("%d expectation(s) failed\n", g_failed);
    else printf("selection_check: all expectations hold\n");
    return g_failed ? 1 : 0;
}
