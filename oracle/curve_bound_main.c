/* Stand-alone driver of the oracle's cost-curve bookkeeping, meant for an address / undefined-behaviour sanitizer build:
 *
 *     cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -ffp-contract=off -mfma -o curve_bound curve_bound_main.c -lm
 *
 * It runs whole episodes of LDE, GLEET, RL-PSO, QLPSO, DE and PSO at budgets whose reference cost list outgrows n_logpoint + 1 entries
 * (include/mbx.h: the curve bound) and prints one line per episode: "<algo> np dim max_fes log_interval n_logpoint steps fes cost_len".  The oracle
 * allocates n_logpoint + 2 curve slots; a write past them is what the sanitizer reports.  tests/test_curve_bound.py builds and runs it. */
#include <stdio.h>

#include "mbx_oracle.c"

typedef struct { int np, dim, max_fes, log_interval, n_logpoint; } budget;

static uint32_t lcg_state = 12345u;
static float lcg01(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) / 16777216.0f; }

static int run(int algo, const char* name, const mbx_problem_desc* p, budget b)
{
    mbx_algo_cfg cfg = {algo, b.np, b.dim, b.max_fes, b.log_interval, b.n_logpoint, 1, 5, 0};
    const int cap = 4 * b.max_fes + 16;
    float act[2 * 256];
    double feat[27 * 256], out3[3] = {0, 0, 0}, fes = 0.;
    int steps = 0, done = 0, cost_len = 0;
    if (algo == MBX_ALGO_LDE) {
        orc_lde* o = orc_lde_new(p, 0., &cfg, 7);
        orc_lde_reset(o, NULL, feat);
        while (!done && steps < cap) {
            for (int i = 0; i < 2 * b.np; ++i) act[i] = lcg01();
            orc_lde_step(o, act, NULL, feat, out3); done = out3[1] != 0.; ++steps;
        }
        fes = o->fes; cost_len = o->cost_len; orc_lde_free(o);
    } else if (algo == MBX_ALGO_GLEET) {
        orc_gleet* o = orc_gleet_new(p, 0., &cfg, 7);
        orc_gleet_reset(o, NULL, feat);
        while (!done && steps < cap) {
            for (int i = 0; i < b.np; ++i) act[i] = lcg01();
            orc_gleet_step(o, act, NULL, feat, out3); done = out3[1] != 0.; ++steps;
        }
        fes = o->fes; cost_len = o->cost_len; orc_gleet_free(o);
    } else if (algo == MBX_ALGO_RLPSO) {
        orc_rlpso* o = orc_rlpso_new(p, 0., &cfg, 7);
        orc_rlpso_reset(o, NULL, feat);
        while (!done && steps < cap) { orc_rlpso_step(o, lcg01() * 1.4f - 0.2f, NULL, feat, out3); done = out3[1] != 0.; ++steps; }
        fes = o->fes; cost_len = o->cost_len; orc_rlpso_free(o);
    } else if (algo == MBX_ALGO_QLPSO) {
        orc_qlpso* o = orc_qlpso_new(p, 0., &cfg, 7);
        orc_qlpso_reset(o, NULL);
        while (!done && steps < cap) { orc_qlpso_step(o, (int)(lcg01() * 4.f) & 3, NULL, out3); done = out3[1] != 0.; ++steps; }
        fes = o->fes; cost_len = o->cost_len; orc_qlpso_free(o);
    } else {
        orc_classic* o = orc_classic_new(p, 0., &cfg, 7);
        orc_classic_reset(o);
        while (!done && steps < cap) { done = orc_classic_step(o); ++steps; }
        fes = o->fes; cost_len = o->cost_len; orc_classic_free(o);
    }
    printf("%s %d %d %d %d %d %d %.0f %d\n", name, b.np, b.dim, b.max_fes, b.log_interval, b.n_logpoint, steps, fes, cost_len);
    return done ? 0 : 1;
}

int main(void)
{
    /* a shifted sphere (kind 1) with an identity map: far from 1e-8 inside these budgets */
    static double dshift[ORC_MAXD], m1[ORC_MAXD * ORC_MAXD];
    /* one entry too long for a kernel that moves the population (4, 2, 29, 5, 5); 52 entries at --maxFEs 976 for one evaluation per step; at least three too long for all */
    const budget budgets[] = {{4, 2, 29, 5, 5}, {30, 10, 976, 19, 50}, {4, 2, 45, 2, 5}, {5, 3, 45, 5, 5}};
    const struct { int algo; const char* name; } algos[] = {{MBX_ALGO_LDE, "lde"}, {MBX_ALGO_GLEET, "gleet"}, {MBX_ALGO_RLPSO, "rlpso"},
                                                           {MBX_ALGO_QLPSO, "qlpso"}, {MBX_ALGO_DE, "de"}, {MBX_ALGO_PSO, "pso"}};
    int bad = 0;
    for (size_t k = 0; k < sizeof budgets / sizeof budgets[0]; ++k) {
        const int D = budgets[k].dim;
        mbx_problem_desc p;
        memset(&p, 0, sizeof p);
        for (int i = 0; i < D; ++i) { dshift[i] = 0.5 + 0.25 * i; for (int j = 0; j < D; ++j) m1[i * D + j] = i == j; }
        p.func_id = 1; p.kind = 1; p.dim = D; p.lb = -5.; p.ub = 5.; p.dshift = dshift; p.m1 = m1;
        for (size_t a = 0; a < sizeof algos / sizeof algos[0]; ++a) bad += run(algos[a].algo, algos[a].name, &p, budgets[k]);
    }
    return bad ? 2 : 0;
}
