// partition_check.cpp -- the partitions of promp_amd/csrc/promp_plan.h (minibatched Adam epochs), checked on the host alone.
//
// Stand-alone: includes the plan header and nothing else of the project.  tests/test_minibatch_host.py compiles it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined
// and runs it once.  One line per failed expectation, exit status 1 if there was any.
//
//   layout       for ragged offsets and several assignments: every minibatch's selection and tables are what build_selection +
//                build_step_tables give for the same index set; the copy table sends every path behind its predecessors of the
//                same minibatch and task, and the destination rows tile [0, R) without gap or overlap
//   table block  pieces on multiples of 64 ints, `total` their sum, and the image reads back as the tables it was packed from
//   refusals     B < 1, an entry outside [0, B), a (minibatch, task) left without a path, B above a task's path count: each with
//                its message, and nothing written (under the sanitizer: without a stray access either)
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

// the ragged batch of tests/subsample_checks.py: 3 tasks with 5, 3 and 4 paths
static const int LEN[12] = {17, 16, 31, 1, 33, 9, 35, 18, 20, 3, 47, 15};
static const int32_t TPO[4] = {0, 5, 8, 12};
static const int M = 3, NP = 12;

static bool same_items(const std::vector<WorkItem>& a, const std::vector<WorkItem>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].task != b[i].task || a[i].row_begin != b[i].row_begin || a[i].row_end != b[i].row_end) return false;
    return true;
}
static bool same_segs(const std::vector<ChainSeg>& a, const std::vector<ChainSeg>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].task != b[i].task || a[i].tile0 != b[i].tile0 || a[i].ntiles != b[i].ntiles) return false;
    return true;
}

// The table block of a partition: pieces on multiples of 64 ints, one behind the other without overlap, `total` their sum; and
// every table read back from the image at the layout's offsets is the StepTables it was packed from.
static void check_block(const PartitionLayout& part, int B, int max_work) {
    const TableBlock blk(NP, B, M, max_work);
    auto r64 = [](size_t n) { return (n + 63) / 64 * 64; };
    // copy table | shifts | B x (tro | two | slot | wg_off | work | segs), each piece rounded up to 64 ints
    const size_t slab_pieces[6] = {(size_t)M + 1, (size_t)M + 1, (size_t)M + 1, (size_t)max_work + 1, 4 * (size_t)max_work, 4 * (size_t)max_work};
    const size_t slab_at[6] = {blk.tro, blk.two, blk.slot, blk.wg_off, blk.work, blk.segs};
    size_t at = 0;
    for (int i = 0; i < 6; ++i) {
        EXPECT(slab_at[i] == at && slab_at[i] % 64 == 0, "piece %d of a slab's part starts at %zu, expected %zu", i, slab_at[i], at);
        at += r64(slab_pieces[i]);
    }
    EXPECT(blk.slab_stride == at, "a slab's part holds %zu ints, its pieces %zu", blk.slab_stride, at);
    EXPECT(blk.shift == r64(2 * NP) && blk.slab0 == blk.shift + r64(B), "copy table and shifts in front of the slabs");
    EXPECT(blk.total == r64(2 * NP) + r64(B) + B * at, "total %zu, the pieces sum to %zu", blk.total, r64(2 * NP) + r64(B) + B * at);
    for (int j = 0; j < B; ++j) EXPECT(blk.slab(j) % 64 == 0 && blk.slab(j) == blk.slab0 + j * blk.slab_stride, "slab %d at %zu", j, blk.slab(j));
    std::vector<int> shifts(B), image(blk.total + 1, -1);
    for (int j = 0; j < B; ++j) shifts[j] = 1000 + 64 * j;
    pack_table_block(blk, part.copy, shifts, part.tables.data(), image.data());
    EXPECT(image[blk.total] == -1, "the image was written past its end");
    EXPECT(std::equal(part.copy.begin(), part.copy.end(), image.begin()), "copy table of the image");
    EXPECT(std::equal(shifts.begin(), shifts.end(), image.begin() + blk.shift), "shifts of the image");
    for (int j = 0; j < B; ++j) {
        const StepTables& t = part.tables[j];
        const int* s = image.data() + blk.slab(j);
        EXPECT(t.tro == std::vector<int>(s + blk.tro, s + blk.tro + M + 1), "slab %d: task row offsets", j);
        EXPECT(t.two[0] == std::vector<int>(s + blk.two, s + blk.two + M + 1), "slab %d: work item offsets", j);
        EXPECT(t.slot_chain == std::vector<int>(s + blk.slot, s + blk.slot + M + 1), "slab %d: chain slot offsets", j);
        EXPECT(t.wg_off == std::vector<int>(s + blk.wg_off, s + blk.wg_off + t.wg_off.size()), "slab %d: workgroup segment offsets", j);
        const WorkItem* w = reinterpret_cast<const WorkItem*>(s + blk.work);
        const ChainSeg* g = reinterpret_cast<const ChainSeg*>(s + blk.segs);
        EXPECT(same_items(t.work[0], std::vector<WorkItem>(w, w + t.work[0].size())), "slab %d: work items", j);
        EXPECT(same_segs(t.segs, std::vector<ChainSeg>(g, g + t.segs.size())), "slab %d: chain segments", j);
        EXPECT((int)t.work[0].size() <= max_work && (int)t.segs.size() <= max_work && (int)t.wg_off.size() <= max_work + 1, "slab %d: tables outgrow their pieces", j);
    }
}

static void check_layout(const std::vector<int32_t>& pro) {
    const int R = pro[NP];
    const std::vector<std::pair<int, std::vector<int32_t>>> cases = {
        {1, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
        {2, {0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1}},      // task 1 keeps one 9-row path in minibatch 0
        {2, {1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0}},
        {3, {0, 1, 2, 1, 0, 2, 0, 1, 0, 1, 2, 2}},      // every share of task 1 a single path
    };
    for (const auto& cs : cases) {
        const int B = cs.first;
        const std::vector<int32_t>& assign = cs.second;
        for (int n_cus : {2, 256}) {
            const int max_work = 2 * n_cus + M;
            PartitionLayout part;
            std::string why;
            const int rc = build_partition(n_cus, max_work, M, NP, TPO, pro.data(), B, assign.data(), &part, &why);
            EXPECT(rc == 0, "B = %d refused: %s", B, why.c_str());
            if (rc) continue;
            EXPECT((int)part.lay.size() == B && (int)part.tables.size() == B && (int)part.row_base.size() == B + 1 && (int)part.copy.size() == 2 * NP,
                   "sizes of the outputs");
            EXPECT(part.row_base[0] == 0 && part.row_base[B] == R, "the slabs hold %d rows, the step %d", part.row_base[B], R);
            std::vector<int> owner(R, -1);
            for (int j = 0; j < B; ++j) {
                std::vector<int32_t> idx;
                for (int p = 0; p < NP; ++p)
                    if (assign[p] == j) idx.push_back(p);
                SelectionLayout lay;
                StepTables t;
                const int n = (int)idx.size();
                int r2 = build_selection(M, NP, TPO, pro.data(), n, idx.data(), &lay, &why);
                EXPECT(r2 == 0, "build_selection refused minibatch %d: %s", j, why.c_str());
                if (r2) continue;
                r2 = build_step_tables(n_cus, max_work, lay.pro[n], n, M, n, lay.tpo.data(), lay.pro.data(), &t, &why);
                EXPECT(r2 == 0, "build_step_tables refused minibatch %d: %s", j, why.c_str());
                if (r2) continue;
                const SelectionLayout& L = part.lay[j];
                const StepTables& T = part.tables[j];
                EXPECT(L.idx == lay.idx && L.tpo == lay.tpo && L.pro == lay.pro, "minibatch %d of %d: the selection differs", j, B);
                EXPECT(T.pro == t.pro && T.tpo == t.tpo && T.path_task == t.path_task && T.row_t == t.row_t && T.tro == t.tro,
                       "minibatch %d of %d: offsets of the tables differ", j, B);
                EXPECT(T.two[0] == t.two[0] && T.two[1] == t.two[1] && T.wg_off == t.wg_off && T.slot_chain == t.slot_chain,
                       "minibatch %d of %d: work offsets differ", j, B);
                EXPECT(same_items(T.work[0], t.work[0]) && same_items(T.work[1], t.work[1]) && same_segs(T.segs, t.segs),
                       "minibatch %d of %d: work tables differ", j, B);
                EXPECT(part.row_base[j + 1] - part.row_base[j] == lay.pro[n], "minibatch %d: %d rows, its paths hold %d", j,
                       part.row_base[j + 1] - part.row_base[j], lay.pro[n]);
                // the copy table: selected path q of minibatch j lands on the slab's rows [pro[q], pro[q + 1])
                for (int q = 0; q < n; ++q) {
                    const int p = idx[q];
                    EXPECT(part.copy[2 * p] == j, "path %d is filed under minibatch %d, assigned %d", p, part.copy[2 * p], j);
                    EXPECT(part.copy[2 * p + 1] == part.row_base[j] + lay.pro[q], "path %d goes to row %d, expected %d", p, part.copy[2 * p + 1],
                           part.row_base[j] + lay.pro[q]);
                }
            }
            for (int p = 0; p < NP; ++p) {
                const int d = part.copy[2 * p + 1];
                EXPECT(d >= 0 && d + LEN[p] <= R, "path %d: destination rows [%d, %d) outside [0, %d)", p, d, d + LEN[p], R);
                if (d < 0 || d + LEN[p] > R) continue;
                for (int r = d; r < d + LEN[p]; ++r) {
                    EXPECT(owner[r] == -1, "row %d is written by paths %d and %d", r, owner[r], p);
                    owner[r] = p;
                }
            }
            int gaps = 0;
            for (int r = 0; r < R; ++r) gaps += owner[r] < 0;
            EXPECT(gaps == 0, "%d of %d destination rows are written by no path (B = %d)", gaps, R, B);
            check_block(part, B, max_work);
        }
    }
}

static void refuse(int B, const std::vector<int32_t>& assign, const char* msg, const std::vector<int32_t>& pro) {
    PartitionLayout part;
    part.row_base = {-7};
    std::string why;
    const int rc = build_partition(2, 7, M, NP, TPO, pro.data(), B, assign.data(), &part, &why);
    EXPECT(rc == -1, "rc %d for a partition that should be refused (%s)", rc, msg);
    EXPECT(why.find(msg) != std::string::npos, "message '%s' does not say '%s'", why.c_str(), msg);
    EXPECT(part.row_base.size() == 1 && part.row_base[0] == -7 && part.lay.empty() && part.tables.empty() && part.copy.empty(),
           "a refused partition wrote its output (%s)", msg);
}

static void check_refusals(const std::vector<int32_t>& pro) {
    const std::vector<int32_t> good = {0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1};
    refuse(0, good, "num_minibatches 0 is below 1", pro);
    refuse(-2, good, "num_minibatches -2 is below 1", pro);
    std::vector<int32_t> bad = good;
    bad[7] = 2;
    refuse(2, bad, "assignment entry 7: minibatch 2 out of range [0, 2)", pro);
    bad = good;
    bad[0] = -1;
    refuse(2, bad, "assignment entry 0: minibatch -1 out of range [0, 2)", pro);
    bad = good;
    bad[5] = 1;                                    // task 1: all three paths in minibatch 1
    refuse(2, bad, "leaves minibatch 0 without a path of task 1", pro);
    bad = {0, 1, 2, 1, 0, 2, 0, 1, 0, 1, 1, 0};    // task 2 has no path in minibatch 2
    refuse(3, bad, "leaves minibatch 2 without a path of task 2", pro);
    refuse(4, good, "num_minibatches 4 exceeds the 3 paths of task 1", pro);
}

int main() {
    std::vector<int32_t> pro(NP + 1, 0);
    for (int p = 0; p < NP; ++p) pro[p + 1] = pro[p] + LEN[p];
    check_layout(pro);
    check_refusals(pro);
    if (g_failed) printf("%d expectation(s) failed\n", g_failed);
    else printf("partition_check: all expectations hold\n");
    return g_failed ? 1 : 0;
}
