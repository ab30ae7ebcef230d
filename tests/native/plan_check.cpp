// Host check of the device-memory plan's arithmetic (poreseq_amd/csrc/ps_plan.h): the numbers DESIGN.md section 3 promises for a
// 309 GB device, matrix_bytes against the formula it replaced, and what share_cut guarantees about the sub-batches it cuts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../poreseq_amd/csrc/ps_plan.h"

using namespace ps;

static long bad = 0;
#define CHECK(cond) do { if (!(cond)) { if (bad++ < 10) printf("line %d: %s\n", __LINE__, #cond); } } while (0)

static unsigned long long rnd_state = 88172645463325252ull;
static unsigned long long rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

// rounded to the digits DESIGN.md prints: whole GB from 10 GB on, one decimal below
static double printed_gb(double bytes) { const double gb = bytes * 1e-9; return gb >= 10 ? std::floor(gb) : std::round(gb * 10) / 10; }

int main(int argc, char** argv) {
    const long trials = argc > 1 ? atol(argv[1]) : 20000;
    // 1. the plan of a 309 GB device
    const size_t dev = (size_t)309e9;
    for (int n = 1; n <= 4; n++) CHECK(printed_gb(share_bytes(dev, n)) == 31);
    CHECK(printed_gb(share_bytes(dev, 7)) == 17);
    CHECK(printed_gb(share_bytes(dev, 14)) == 7.7);
    for (int n : {1, 4, 7, 14, 30}) {   // share = (0.60 x device / threads - 2.5 GB) / 1.4, at least four threads, at least 2 GB
        const double want = std::fmax(2e9, (0.60 * 309e9 / (n < 4 ? 4 : n) - 2.5e9) / 1.4);
        CHECK(std::fabs(share_bytes(dev, n) - want) <= 1e-6 * want);
    }
    CHECK(share_bytes(dev, 40) == 2e9 && share_bytes(dev, 1000) == 2e9 && share_bytes((size_t)10e9, 4) == 2e9);   // the floor
    CHECK(share_bytes(dev, 30) > 2e9);
    // 27 % slabs + 60 % runtimes leave 13 %
    CHECK(PLAN_SLABS == 3 && slab_default_bytes(dev) == (size_t)(0.09 * 309e9));
    CHECK(std::fabs(1.0 - PLAN_SLABS * PLAN_SLAB_FRAC - PLAN_RUNTIMES_FRAC - 0.13) < 1e-12);
    CHECK(PLAN_RUNTIMES_FRAC == 0.60 && PLAN_PER_SHARE == 1.4 && PLAN_FIXED_BYTES == 2.5e9 && PLAN_SHARE_FLOOR == 2e9 && PLAN_MIN_RUNTIMES == 4);
    CHECK(PLAN_POOL_CEILING == 0.94 && PLAN_MATRIX_CEILING == 0.92 && PLAN_OVER_GUESS == 1.2 && PLAN_SW_PART == 8 && PLAN_VITERBI_FRAC == 0.9);
    CHECK(align_cache_default(dev) == (size_t)8e9);                          // 3 % of 309 GB = 9.3 GB: the 8 GB bound holds
    CHECK(align_cache_default((size_t)100e9) == (size_t)(0.03 * 100e9));     // a rank with a third of the device: 3 %
    CHECK(align_cache_default((size_t)8e9 * 100 / 3 + 1000) == (size_t)8e9);
    // 2. matrix bytes: (S + MAT_FRONT + MAT_BACK) * P * 18, per direction
    CHECK(MAT_FRONT == 8 && MAT_BACK == 16 && PS_CELL_BYTES == 18);
    const long long shapes[][2] = {{1, 64}, {20001, 192}, {20001, 1024}, {60000, 2048}, {12345, 320}, {301, 64}};
    for (const auto& s : shapes) {
        const long long S = s[0], P = s[1];
        CHECK(matrix_cells(S, (int)P) == (S + 8 + 16) * P);
        CHECK(matrix_bytes(S, (int)P, 1) == (double)((S + 8 + 16) * P * 18));
        CHECK(matrix_bytes(S, (int)P, 2) == (double)((S + 8 + 16) * P * 36));
        CHECK(matrix_bytes(S, (int)P, 1) == ((double)S + MAT_FRONT + MAT_BACK) * P * 18.0);          // as fwd_job_bytes wrote it
        CHECK(matrix_bytes(S, (int)P, 2) == ((double)S + MAT_FRONT + MAT_BACK) * P * 18.0 * 2);      // as fit_share wrote it
        CHECK(matrix_bytes(S, (int)P, 2) == ((double)S + MAT_FRONT + MAT_BACK) * P * 36.0);          // as the lone-region estimate wrote it
    }
    // the guesses of P: W = 150 (the default realign_width) -> 301 / 1.9 + 9 = 167 -> 192 slots; never under 64, never over 1024
    CHECK(guess_slots_w(150) == 192 && guess_slots_w(0) == 64 && guess_slots_w(5000) == 1024);
    CHECK(most_slots_w(150) == 374 && most_slots_w(5000) == 1024);
    for (int W = 0; W < 600; W++) CHECK(guess_slots_w(W) % 64 == 0 && guess_slots_w(W) <= std::max(64, most_slots_w(W)));
    // 3. share_cut over random lists
    for (long it = 0; it < trials; it++) {
        const size_t n = 1 + rnd() % 40;
        std::vector<double> need(n);
        const double scale = it % 3 == 0 ? 1e9 : (it % 3 == 1 ? 30e9 : 5e9);
        for (double& v : need) v = (double)(rnd() % 1000 + (it % 7 == 0 ? 0 : 1)) * 1e-3 * scale;   // (now and then items of no bytes)
        const double cap = (double)(rnd() % 1000 + 1) * 1e-3 * 20e9;
        auto f = [&](size_t k) { return need[k]; };
        double total = 0;
        for (double v : need) total += v;
        if (total <= cap) CHECK(share_cut(0, n, cap, f) == n);           // a list that fits is one chunk
        size_t k0 = 0, chunks = 0;
        while (k0 < n) {
            const size_t k1 = share_cut(k0, n, cap, f);
            CHECK(k1 > k0 && k1 <= n);                                     // always advances, never past the end
            if (k1 <= k0) break;
            double sum = 0;
            for (size_t k = k0; k < k1; k++) sum += need[k];
            if (k1 - k0 > 1) CHECK(sum <= cap);                            // only a lone item may exceed the cap
            k0 = k1;                                                       // (the next chunk starts where this one ended: every index once, in order)
            chunks++;
        }
        CHECK(k0 == n && chunks <= n);
    }
    CHECK(share_cut(3, 3, 1e9, [](size_t) { return 1.0; }) == 3);         // nothing left: nothing cut
    // 4. greedy_cut (the chunks of candidate-sequence alignments): in order, as many as the cap holds, at most `limit`, at least one
    {
        const std::vector<double> need = {3, 4, 5, 20, 1, 1, 8, 2};
        auto f = [&](size_t k) { return need[k]; };
        const size_t n = need.size(), any = (size_t)-1;
        CHECK(greedy_cut(0, n, 44, any, f) == n && greedy_cut(0, n, 1e9, any, f) == n);   // everything fits (3 + ... + 2 = 44)
        CHECK(greedy_cut(0, n, 1e9, 1, f) == 1 && greedy_cut(3, n, 1e9, 1, f) == 4);      // a limit of 1: one item, whatever the cap
        CHECK(greedy_cut(0, n, 1e9, 3, f) == 3 && greedy_cut(6, n, 1e9, 3, f) == n);      // (a limit past the end: the end)
        CHECK(greedy_cut(3, n, 10, any, f) == 4);                                         // an item larger than the cap goes alone
        CHECK(greedy_cut(0, n, 10, any, f) == 2 && greedy_cut(2, n, 10, any, f) == 3);    // ... and does not join the items before it
        CHECK(greedy_cut(0, n, 12, any, f) == 3);                                         // 3 + 4 + 5 lands exactly on the cap: all three
        CHECK(greedy_cut(0, n, 11.999, any, f) == 2);
        CHECK(greedy_cut(4, n, 10, any, f) == 7 && greedy_cut(4, n, 10, 2, f) == 6);      // q0 in the middle: 1 + 1 + 8 from there, or the limit
        CHECK(greedy_cut(n, n, 10, any, f) == n);                                         // nothing left: nothing cut
        size_t calls = 0;                                                                  // every item is sized once, and the one that ends the chunk
        CHECK(greedy_cut(0, n, 10, any, [&](size_t k) { calls++; return need[k]; }) == 2 && calls == 3);
    }
    for (long it = 0; it < trials; it++) {   // against a literal restatement, over random lists
        const size_t n = 1 + rnd() % 30, q0 = rnd() % n, limit = it % 4 == 0 ? (size_t)-1 : 1 + rnd() % 8;
        std::vector<double> need(n);
        for (double& v : need) v = (double)(rnd() % 64);
        const double cap = (double)(rnd() % 256);
        size_t want = q0 + 1;
        double sum = need[q0];
        while (want < n && want - q0 < limit && sum + need[want] <= cap) sum += need[want++];
        CHECK(greedy_cut(q0, n, cap, limit, [&](size_t k) { return need[k]; }) == want);
    }
    printf("failures=%ld\n", bad);
    return bad != 0;
}
