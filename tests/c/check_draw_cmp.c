/* Checks dm_draw_compare (include/eslam_detmath.h), the integer decision "T_k* <= c", against
 * the definition of the stratified draws: T_k = dm_fx_shift(((double)k + dm_minstd_uniform(x_k))
 * / N, shift) and dm_count_draws_le.  Test infrastructure: built and run by
 * tests/test_draw_compare.py.
 *
 *   check_draw_cmp <iterations>
 *
 * For every N of the list, both supported production shifts (60: the update path, 61: a
 * stand-alone resample's upper end) and <iterations> rounds, the draws (k, x) are: a random k
 * with a random x, with x = 1 and with x = 2147483646, and k = 0 and k = N - 1 each with a
 * random x and with the x edge (seven per round).  The minstd start is chosen so that draw k
 * has state x; the state handed to the decision is that of k* = floor(c N / 2^shift) of each
 * target, which is k or (edge targets) a neighbour.  Targets c per draw:
 *   edge     T - 1, T, T + 1 and the four thresholds of the decision -- k 2^shift / N + m,
 *            (k + 1) 2^shift / N - m, R - m, R + m with R = floor((k + u) 2^shift / N) --
 *            each with - 1, + 0, + 1 (negative ones do not exist as targets)
 *   random   one uniform in the stratum [ceil(k 2^shift / N), ceil((k + 1) 2^shift / N))
 * Checked: every certain answer equals T_k* <= c and k* + answer equals dm_count_draws_le;
 * |T - R| < m = dm_draw_margin(shift); no random target is ambiguous.  A random target is
 * ambiguous with probability below 4 m N / 2^shift (2^-17 at N = 2^32 - 1, 2^-23 at 2^26), so
 * the fixed-seed sample of the test (1500 rounds: 10 500 random targets per N and shift) is
 * expected to hold 0.08 of them at the largest N, and holds none (the seed is fixed, so the
 * sample never changes).
 * Prints the counts; exit status 1 on any failure.                                          */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "eslam_detmath.h"

typedef unsigned __int128 u128;
typedef __int128 i128;

static uint64_t sm_state = 0x9E3779B97F4A7C15ull;
static uint64_t splitmix(void)
{
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t wrong = 0, bound_bad = 0, certain_n = 0, ambiguous_n = 0;
static uint64_t random_n = 0, random_ambiguous = 0, edge_n = 0, edge_ambiguous = 0, worst_dev = 0;

static uint64_t draw_T(uint64_t k, uint32_t x, uint64_t N, int shift)
{
    return dm_fx_shift(((double)k + dm_minstd_uniform(x)) / (double)N, shift);
}

/* the state of draw k after the start xs (the (k + 1)-th minstd step) */
static uint32_t state_of(uint64_t k, uint32_t xs) { return dm_mulmod31(dm_minstd_pow(k + 1), xs); }

/* the start for which draw k has state x: x A^-(k+1), A^(p-1) = 1 mod p */
static uint32_t start_for(uint64_t k, uint32_t x)
{
    const uint64_t e = (k + 1) % 2147483646ull;
    return dm_mulmod31(x, dm_minstd_pow(2147483646ull - e));
}

static void check_target(i128 cs, uint64_t N, uint32_t xs, int shift, int is_random)
{
    if (cs < 0 || cs >= ((i128)1 << 62)) return;
    const uint64_t c = (uint64_t)cs;
    const uint64_t kstar = (uint64_t)(((u128)c * N) >> shift);
    const uint32_t x = state_of(kstar, xs);
    const int d = dm_draw_compare(c, N, x, shift);
    if (is_random) ++random_n; else ++edge_n;
    if (d == DM_DRAW_AMBIGUOUS) {
        ++ambiguous_n;
        if (is_random) {
            if (random_ambiguous < 10) fprintf(stderr, "random target ambiguous: c=%llu N=%llu x=%u shift=%d\n",
                                               (unsigned long long)c, (unsigned long long)N, x, shift);
            ++random_ambiguous;
        } else {
            ++edge_ambiguous;
        }
        return;
    }
    ++certain_n;
    int ok = kstar < N && (d == DM_DRAW_LE || d == DM_DRAW_GT);
    if (ok) ok = (draw_T(kstar, x, N, shift) <= c) == (d == DM_DRAW_LE);
    if (ok) ok = dm_count_draws_le(c, N, xs, shift) == kstar + (uint64_t)d;
    if (!ok) {
        if (wrong < 10) fprintf(stderr, "wrong decision %d: c=%llu N=%llu k*=%llu x=%u shift=%d\n", d, (unsigned long long)c,
                                (unsigned long long)N, (unsigned long long)kstar, x, shift);
        ++wrong;
    }
}

static void check_draw(uint64_t k, uint32_t x, uint64_t N, int shift)
{
    const uint32_t xs = start_for(k, x);
    if (state_of(k, xs) != x) { fprintf(stderr, "start_for is wrong\n"); exit(2); }
    const uint64_t m = dm_draw_margin(shift);
    const uint64_t T = draw_T(k, x, N, shift);
    /* R = floor((k + u) 2^shift / N), u = (x - 1) / 2147483646: (k M + x - 1) 2^shift / (N M) */
    const u128 num = ((u128)k * 2147483646u + (x - 1u)) << shift;
    const uint64_t R = (uint64_t)(num / ((u128)N * 2147483646u));
    const uint64_t dev = T > R ? T - R : R - T;
    if (dev > worst_dev) worst_dev = dev;
    if (dev >= m) {
        if (bound_bad < 10) fprintf(stderr, "|T - R| = %llu >= m: k=%llu x=%u N=%llu shift=%d\n", (unsigned long long)dev,
                                    (unsigned long long)k, x, (unsigned long long)N, shift);
        ++bound_bad;
    }
    const i128 s_lo = (i128)((((u128)k << shift) + N - 1) / N);             /* ceil(k 2^shift / N) */
    const i128 s_hi = (i128)(((((u128)k + 1) << shift) + N - 1) / N);       /* ceil((k + 1) 2^shift / N) */
    const i128 thr[5] = {(i128)T, (i128)(((u128)k << shift) / N) + (i128)m, (i128)((((u128)k + 1) << shift) / N) - (i128)m,
                         (i128)R - (i128)m, (i128)R + (i128)m};
    for (int t = 0; t < 5; ++t)
        for (int o = -1; o <= 1; ++o) check_target(thr[t] + o, N, xs, shift, 0);
    if (s_hi > s_lo) check_target(s_lo + (i128)(splitmix() % (uint64_t)(s_hi - s_lo)), N, xs, shift, 1);
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: check_draw_cmp <iterations>\n"); return 2; }
    const uint64_t iters = strtoull(argv[1], NULL, 10);
    static const uint64_t Ns[] = {1, 2, 3, 63, 64, 65, 4096, 1ull << 22, (1ull << 22) + 1, 1ull << 26, 4294967295ull};
    static const int shifts[] = {60, 61};
    for (unsigned a = 0; a < sizeof(Ns) / sizeof(Ns[0]); ++a) {
        const uint64_t N = Ns[a];
        for (unsigned b = 0; b < 2; ++b) {
            const int shift = shifts[b];
            for (uint64_t t = 0; t < iters; ++t) {
                const uint64_t k = splitmix() % N;
                const uint32_t x = 1 + (uint32_t)(splitmix() % 2147483646u);
                check_draw(k, x, N, shift);
                check_draw(k, 1u, N, shift);
                check_draw(k, 2147483646u, N, shift);
                check_draw(0, x, N, shift);
                check_draw(0, 1u, N, shift);
                check_draw(N - 1, x, N, shift);
                check_draw(N - 1, 2147483646u, N, shift);
            }
        }
    }
    /* shifts, targets and counts outside the decision's domain are ambiguous */
    uint64_t domain_bad = 0;
    for (int shift = 0; shift <= 64; ++shift)
        if (!dm_draw_shift_ok(shift) && dm_draw_compare(1ull << 40, 4096, 12345u, shift) != DM_DRAW_AMBIGUOUS) ++domain_bad;
    if (dm_draw_compare(1ull << 62, 4096, 12345u, 60) != DM_DRAW_AMBIGUOUS) ++domain_bad;
    if (dm_draw_compare(1ull << 40, 1ull << 32, 12345u, 60) != DM_DRAW_AMBIGUOUS) ++domain_bad;
    if (dm_draw_compare(1ull << 40, 0, 12345u, 60) != DM_DRAW_AMBIGUOUS) ++domain_bad;
    if (dm_draw_compare(1ull << 60, 4096, 12345u, 60) != DM_DRAW_AMBIGUOUS) ++domain_bad;      /* k* = N */
    printf("%llu certain, %llu ambiguous, %llu wrong decisions, %llu bound violations (worst |T - R| %llu), "
           "%llu edge targets (%llu ambiguous), %llu random targets, %llu random ambiguous, %llu domain failures\n",
           (unsigned long long)certain_n, (unsigned long long)ambiguous_n, (unsigned long long)wrong,
           (unsigned long long)bound_bad, (unsigned long long)worst_dev, (unsigned long long)edge_n,
           (unsigned long long)edge_ambiguous, (unsigned long long)random_n, (unsigned long long)random_ambiguous,
           (unsigned long long)domain_bad);
    return (wrong || bound_bad || random_ambiguous || domain_bad || certain_n == 0 || edge_ambiguous == 0) ? 1 : 0;
}
