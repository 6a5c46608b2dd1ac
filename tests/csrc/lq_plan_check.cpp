// TEST INFRASTRUCTURE ONLY.  A stand-alone program around cut_lq_jobs / next_poa_slice (csrc/nd_lqplan.h), the arithmetic that cuts a
// low-quality-region round into K12a's jobs and a POA round into launches: built with -fsanitize=address,undefined by
// tests/test_lq_plan.py and run directly.  The expectation is the two loops as run_lq and run_poa had them inline (old_cut_jobs,
// old_slices: restated verbatim on plain records); 2,000 seeded draws each are compared field by field, five fixed cases have their
// answers written out; the first failure is printed and the exit status is 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nd_lqplan.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // splitmix64: the draws are the same on every machine
    uint64_t x = (g_state += 0x9e3779b97f4a7c15ull);
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
uint64_t between(uint64_t lo, uint64_t hi) { return lo + rnd() % (hi - lo + 1); }

// ---- the job cutter as run_lq had it: a round's pieces (row-major, 30 rows x nr regions), its jobs, the call's job list ----
struct Job { int q_len, t_len; };
struct Piece { int job; unsigned sl; };
struct Round { std::vector<Piece> pieces; std::vector<Job> jobs; };
struct JobDev { uint32_t pile, g_a, g_b, t0, t1, row_cap, lnk_cap; uint64_t hdr_off, lnk_off; };

void old_cut_jobs(const Round &R, uint32_t nr, size_t r, uint64_t job_cols, uint64_t &hdr_words, uint64_t &lnk_words, std::vector<JobDev> &jobs) {
    uint32_t g = 0, t = 0;
    while (g < nr) {
        JobDev jb;
        memset(&jb, 0, sizeof(jb));
        jb.pile = (uint32_t)r, jb.g_a = g, jb.t0 = t;
        uint64_t cols = 0, ins = 0, tags = 0;
        do {
            const uint32_t sl = R.pieces[g].sl;
            cols += (uint64_t)sl + 1;
            tags += 30;
            for (uint32_t row = 0; row < 30u; row++) {
                const Piece &pc = R.pieces[(size_t)row * nr + g];
                if (pc.job >= 0) {
                    const Job &j = R.jobs[(size_t)pc.job];
                    ins += (uint64_t)j.q_len;
                    tags += (uint64_t)j.q_len + (uint64_t)j.t_len;
                } else tags += sl;
            }
            t += sl + 1;
            g++;
        } while (g < nr && (cols < job_cols || R.pieces[g - 1].sl == 0));
        jb.g_b = g;
        if (g == nr) cols += 1, tags += 30, t += 1;  // the closing 'N'
        jb.t1 = t;
        jb.row_cap = (uint32_t)std::min<uint64_t>(cols + ins, 3 * cols + 256);
        jb.lnk_cap = (uint32_t)std::min<uint64_t>(tags, (uint64_t)jb.row_cap * 30u);
        jb.hdr_off = hdr_words, jb.lnk_off = lnk_words;
        hdr_words += jb.row_cap;
        lnk_words += jb.lnk_cap;
        jobs.push_back(jb);
    }
}

// What layout_lq_round hands the cutter: per region its length, the sums over the rows that have a job, the rows that have none.
std::vector<ndgpu::LqRegionLoad> loads_of(const Round &R, uint32_t nr) {
    std::vector<ndgpu::LqRegionLoad> load(nr);
    for (uint32_t g = 0; g < nr; g++) load[g] = ndgpu::LqRegionLoad{R.pieces[g].sl, 0, 0, 0};
    for (size_t k = 0; k < R.pieces.size(); k++) {
        ndgpu::LqRegionLoad &L = load[k % nr];
        if (R.pieces[k].job < 0) L.empty_rows++;
        else {
            const Job &j = R.jobs[(size_t)R.pieces[k].job];
            L.q_bases += (uint64_t)j.q_len, L.qt_bases += (uint64_t)j.q_len + (uint64_t)j.t_len;
        }
    }
    return load;
}

Round make_round(const std::vector<uint32_t> &sl, const std::vector<uint32_t> &rows_with_job) {
    const uint32_t nr = (uint32_t)sl.size();
    Round R;
    R.pieces.assign((size_t)30 * nr, Piece{-1, 0});
    for (uint32_t row = 0; row < 30; row++)
        for (uint32_t g = 0; g < nr; g++) {
            Piece &pc = R.pieces[(size_t)row * nr + g];
            pc.sl = sl[g];
            if (row < rows_with_job[g]) {
                pc.job = (int)R.jobs.size();
                R.jobs.push_back(Job{(int)between(1, 6000), (int)sl[g]});
            }
        }
    return R;
}

int compare_jobs(const char *name, int draw, const Round &R, uint32_t nr, uint64_t job_cols, uint64_t hdr0, uint64_t lnk0) {
    uint64_t hdr_a = hdr0, lnk_a = lnk0, hdr_b = hdr0, lnk_b = lnk0;
    std::vector<JobDev> want;
    std::vector<ndgpu::LqJobCut> got;
    old_cut_jobs(R, nr, 0, job_cols, hdr_a, lnk_a, want);
    ndgpu::cut_lq_jobs(loads_of(R, nr), job_cols, 30, hdr_b, lnk_b, got);
    bool ok = want.size() == got.size() && hdr_a == hdr_b && lnk_a == lnk_b;
    for (size_t k = 0; ok && k < want.size(); k++) {
        const JobDev &w = want[k];
        const ndgpu::LqJobCut &c = got[k];
        ok = w.g_a == c.g_a && w.g_b == c.g_b && w.t0 == c.t0 && w.t1 == c.t1 && w.row_cap == c.row_cap && w.lnk_cap == c.lnk_cap &&
             w.hdr_off == c.hdr_off && w.lnk_off == c.lnk_off;
    }
    if (!ok) printf("%s %d: cut_lq_jobs differs from the loop it replaces (%zu jobs, %zu wanted)\n", name, draw, got.size(), want.size());
    return ok ? 0 : 1;
}

int check_job_draw(int draw) {
    const uint32_t nr = (uint32_t)between(1, 200);
    std::vector<uint32_t> sl(nr), rows(nr);
    for (uint32_t g = 0; g < nr;) {  // lengths 0..4,000, a fifth of the stretches a run of zeros (the `sl == 0` continuation rule)
        const bool zeros = between(0, 4) == 0;
        for (uint32_t run = (uint32_t)between(1, zeros ? 6 : 3); run && g < nr; run--, g++) sl[g] = zeros ? 0u : (uint32_t)between(0, 4000);
    }
    for (uint32_t g = 0; g < nr; g++) rows[g] = sl[g] ? (uint32_t)between(0, 30) : 0u;  // (a region without columns has nothing to align)
    const uint64_t job_cols[3] = {1, 40, 192};
    return compare_jobs("draw", draw, make_round(sl, rows), nr, job_cols[draw % 3], between(0, 1u << 20), between(0, 1u << 24));
}

int check_job_fixed(const char *name, const std::vector<uint32_t> &sl, uint64_t job_cols, const std::vector<ndgpu::LqJobCut> &want, uint64_t hdr_end,
                    uint64_t lnk_end) {
    const Round R = make_round(sl, std::vector<uint32_t>(sl.size(), 0));  // (no row has a job: the capacities follow from the lengths)
    if (compare_jobs(name, 0, R, (uint32_t)sl.size(), job_cols, 0, 0)) return 1;
    uint64_t hdr = 0, lnk = 0;
    std::vector<ndgpu::LqJobCut> got;
    ndgpu::cut_lq_jobs(loads_of(R, (uint32_t)sl.size()), job_cols, 30, hdr, lnk, got);
    bool ok = got.size() == want.size() && hdr == hdr_end && lnk == lnk_end;
    for (size_t k = 0; ok && k < got.size(); k++) ok = !memcmp(&got[k], &want[k], sizeof(want[k]));
    if (!ok) printf("%s: not the jobs written out\n", name);
    return ok ? 0 : 1;
}

// ---- the slice cut as run_poa had it: from problem a of the round on ----
struct Prob { uint64_t cells, rows; bool live; };

size_t old_slice(std::vector<Prob> &probs, size_t a, uint64_t budget, std::vector<size_t> &slice) {
    slice.clear();
    uint64_t cells = 0;
    for (; a < probs.size(); a++) {
        Prob &p = probs[a];
        if (p.cells > budget || p.rows > 65535) {
            p.live = false;
            continue;
        }
        if (!slice.empty() && cells + p.cells > budget) break;
        cells += p.cells;
        slice.push_back(a);
    }
    return a;
}

int compare_slices(const char *name, int draw, const std::vector<ndgpu::PoaLoad> &load, uint64_t budget, std::vector<std::vector<size_t>> *slices_out) {
    std::vector<Prob> probs;
    for (const ndgpu::PoaLoad &l : load) probs.push_back(Prob{l.cells, l.rows, true});
    std::vector<uint8_t> live(load.size(), 1);
    std::vector<size_t> want, got, dropped;
    for (size_t a = 0, b = 0; a < load.size() || b < load.size();) {
        a = old_slice(probs, a, budget, want);
        b = ndgpu::next_poa_slice(load, b, budget, got, dropped);
        for (size_t k : dropped) live[k] = 0;
        if (a != b || want != got) {
            printf("%s %d: next_poa_slice differs from the loop it replaces\n", name, draw);
            return 1;
        }
        if (slices_out) slices_out->push_back(got);
    }
    for (size_t k = 0; k < load.size(); k++)
        if ((live[k] != 0) != probs[k].live) {
            printf("%s %d: problem %zu dropped by one cut and not by the other\n", name, draw, k);
            return 1;
        }
    return 0;
}

int check_slice_draw(int draw) {
    const uint64_t budget = draw % 50 == 0 ? 0 : between(1, 200000);
    std::vector<ndgpu::PoaLoad> load((size_t)between(1, 80));
    for (ndgpu::PoaLoad &l : load) {  // cells from 1 to twice the budget, small in half of the problems (several to a slice); rows around 65,535 in a fifth
        l.cells = between(0, 1) ? between(1, 2 * budget + 1) : between(1, budget / 8 + 1);
        l.rows = between(0, 4) ? between(1, 3000) : between(65530, 65540);
    }
    return compare_slices("slice draw", draw, load, budget, nullptr);
}

}  // namespace

int main() {
    for (int draw = 0; draw < 2000; draw++)
        if (check_job_draw(draw) || check_slice_draw(draw)) return 1;
    // a round of one region without columns: the two 'N' columns are its job -- 2 cell rows, 30 tags each
    if (check_job_fixed("one empty region", {0}, 192, {{0, 1, 0, 2, 2, 60, 0, 0}}, 2, 60)) return 1;
    // the last region closes exactly at job_cols (20 + 20 columns of 40): one job, the closing 'N' is its 41st column
    if (check_job_fixed("closes at job_cols", {19, 19}, 40, {{0, 2, 0, 41, 41, 1230, 0, 0}}, 41, 1230)) return 1;
    // the first region closes exactly at job_cols: the second one is a job of its own, behind the first one's streams
    if (check_job_fixed("cut at job_cols", {39, 7}, 40, {{0, 1, 0, 40, 40, 1200, 0, 0}, {1, 2, 40, 49, 9, 270, 40, 1200}}, 49, 1470)) return 1;
    // a region without columns does not end a job, though the job has its 40 columns with it: the cut comes behind the next region that has some
    if (check_job_fixed("zero run", {38, 0, 0, 7, 5}, 40, {{0, 4, 0, 49, 49, 1470, 0, 0}, {4, 5, 49, 56, 7, 210, 49, 1470}}, 56, 1680)) return 1;
    // the first problem alone exceeds the budget: it is dropped, the cut goes on and fills the first launch behind it
    std::vector<std::vector<size_t>> slices;
    if (compare_slices("over budget", 0, {{101, 5}, {50, 5}, {50, 5}, {10, 5}, {10, 65536}}, 100, &slices)) return 1;
    if (slices != std::vector<std::vector<size_t>>{{1, 2}, {3}}) {
        printf("over budget: not the slices written out\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
