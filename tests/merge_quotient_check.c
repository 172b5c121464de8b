/* Test helper (CPU): the greedy scan's one-division merge quotient (sylber_amd/csrc/segment.hip merge_update)
 *     r = RN(1 / c1),  q0 = a r,  q <- fma(fma(-q, c1, a), r, q)  twice
 * against the IEEE division a / c1, for every divisor c1 in {2..8192} and every 7th of 8193..20000 (seg_cnt is never reset inside a
 * run of speech, so a long utterance divides by more than 8192) and dividends a inside [2^-100, 2^126], where the kernel uses it.
 * Per divisor and sign: `per` dividends with a random mantissa in a random binade of the whole range, `per` in the binades activations
 * live in (2^-12 .. 2^16), and `per` built to be hard for a division: a = RN(c1 (q + ulp(q) / 2)) and its two neighbours, whose
 * quotients lie next to a rounding boundary.
 * usage: merge_quotient_check <per>      prints "<dividends checked> <mismatches> <first bad divisor or 0>" */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline uint64_t rng(uint64_t *s) { *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17; return *s; }

static inline float one_division(float a, float c1, float r)
{
    const float q0 = a * r;
    const float q1 = fmaf(fmaf(-q0, c1, a), r, q0);
    return fmaf(fmaf(-q1, c1, a), r, q1);
}

static inline int check(float a, float c1, float r)
{
    if (!(fabsf(a) >= 0x1p-100f) || !(fabsf(a) <= 0x1p126f)) return 0;   /* the kernel's fallback: plain division */
    return f2u(one_division(a, c1, r)) != f2u(a / c1);
}

int main(int argc, char **argv)
{
    long per = argc > 1 ? strtol(argv[1], 0, 10) : 2000;
    unsigned long bad = 0, n = 0;
    long first_bad = 0;
    static int divs[12000];
    int nd = 0;
    for (int c = 2; c <= 8192; c++) divs[nd++] = c;
    for (int c = 8193; c <= 20000; c += 7) divs[nd++] = c;
#pragma omp parallel for reduction(+:bad,n) schedule(dynamic, 16)
    for (int di = 0; di < nd; di++) {
        const float c1 = (float)divs[di];
        const float r = 1.0f / c1;
        uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(divs[di] + 1);
        unsigned long b = 0;
        for (long i = 0; i < per; i++) {
            uint32_t m = (uint32_t)(rng(&s) & 0x7fffffu), sg = (uint32_t)(rng(&s) & 1u) << 31;
            uint32_t e_all = 27 + (uint32_t)(rng(&s) % 226);               /* 2^-100 .. 2^125 */
            uint32_t e_act = 115 + (uint32_t)(rng(&s) % 28);               /* 2^-12 .. 2^15 */
            b += check(u2f(sg | (e_all << 23) | m), c1, r);
            b += check(u2f(sg | (e_act << 23) | m), c1, r);
            /* next to a rounding boundary of the quotient */
            float q = u2f(sg | (e_act << 23) | (uint32_t)(rng(&s) & 0x7fffffu));
            double qm = (double)q + 0.5 * ((double)u2f(f2u(q) + 1) - (double)q);
            float a = (float)(qm * (double)c1);
            b += check(a, c1, r);
            b += check(u2f(f2u(a) + 1), c1, r);
            b += check(u2f(f2u(a) - 1), c1, r);
            n += 5;
        }
        /* the ends of the range the kernel uses it on */
        b += check(0x1p-100f, c1, r) + check(-0x1p-100f, c1, r) + check(0x1p126f, c1, r) + check(-0x1p126f, c1, r);
        b += check(u2f(f2u(0x1p-100f) + 1), c1, r) + check(u2f(f2u(0x1p126f) - 1), c1, r);
        n += 6;
        if (b) {
#pragma omp critical
            if (!first_bad || divs[di] < first_bad) first_bad = divs[di];
        }
        bad += b;
    }
    printf("%lu %lu %ld\n", n, bad, first_bad);
    return bad != 0;
}
