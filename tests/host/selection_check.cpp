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
//   copy table   -1 exactly at the paths not selected, the slab's offsets at the others; a full selection's is the partition's
//                with B = 1; the table block of one slab reads back as the tables it was packed from
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
        // the copy table of the launch that fills the slab: -1 exactly at the paths not selected, the slab's own offsets at the others
        const std::vector<int> copy = selection_copy_table(12, lay);
        EXPECT((int)copy.size() == 24, "copy table of %d ints", (int)copy.size());
        if (copy.size() == 24) {
            for (int p = 0, q = 0; p < 12; ++p) {
                const bool in = q < n && sel[q] == p;
                EXPECT(copy[2 * p] == (in ? 0 : -1), "path %d (%s): slab %d", p, in ? "selected" : "not selected", copy[2 * p]);
                if (in) {
                    EXPECT(copy[2 * p + 1] == lay.pro[q], "path %d goes to row %d, the slab's offset is %d", p, copy[2 * p + 1], lay.pro[q]);
                    ++q;
                }
            }
            if (n == 12) {      // every path selected: the partition into one minibatch
                PartitionLayout part;
                const std::vector<int32_t> assign(12, 0);
                const int prc = build_partition(2, 7, 3, 12, TPO, pro.data(), 1, assign.data(), &part, &why);
                EXPECT(prc == 0 && part.copy == copy, "a full selection's copy table is not the identity partition's (%s)", why.c_str());
            }
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
            // the selection's table block: the partition's shape with one slab, read back whole
            const TableBlock blk(12, 1, 3, 2 * n_cus + 3);
            std::vector<int> image(blk.total, -1);
            pack_table_block(blk, copy, {0}, &t, image.data());
            EXPECT(std::equal(copy.begin(), copy.end(), image.begin()) && image[blk.shift] == 0, "copy table / shift of the image");
            const int* s = image.data() + blk.slab(0);
            EXPECT(blk.slab(0) % 64 == 0 && blk.total == blk.slab(0) + blk.slab_stride, "one slab behind the copy table and the shifts");
            EXPECT(std::equal(t.tro.begin(), t.tro.end(), s + blk.tro) && std::equal(t.two[0].begin(), t.two[0].end(), s + blk.two) &&
                   std::equal(t.slot_chain.begin(), t.slot_chain.end(), s + blk.slot) && std::equal(t.wg_off.begin(), t.wg_off.end(), s + blk.wg_off),
                   "offset tables of the image");
            EXPECT(memcmp(s + blk.work, t.work[0].data(), sizeof(WorkItem) * t.work[0].size()) == 0 &&
                   memcmp(s + blk.segs, t.segs.data(), sizeof(ChainSeg) * t.segs.size()) == 0, "work / segment tables of the image");
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
