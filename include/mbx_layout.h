/*
 * mbx_layout.h — data layouts that are part of the C-ABI contract (shared by libmbx.so, its host
 * mirror and the test oracle; it defines formats only, no algorithm).
 *
 *  1. the per-step "tape" of external random numbers (mbx_set_tape),
 *  2. the per-instance optimizer state exposed by mbx_debug_read_state,
 *  3. the Philox4x32-10 draw-site map (which counter produces which random number).
 *
 * All sizes are in doubles; NP = population size, D = dimension.
 */
#ifndef MBX_LAYOUT_H
#define MBX_LAYOUT_H

#include <stdint.h>

/* ---------------------------------------------------------------- 1. RLEPSO tape (per instance, per step)
 * Slots follow the draw order of RLEPSO_Optimizer.update (reference: rlepso_optimizer.py:179-180,
 * 77,88,108, eval noise, 238, 137-138, eval noise):
 *   rand1[NP] rand2[NP] clpso_u[NP*D] tourn_idx[NP*D*2] fdr_u[NP*D] noise_main[3*NP]
 *   reinit_u[NP] reinit_pos_u[NP*D] reinit_vel_u[NP*D] noise_reinit[3*NP]
 * Every value is the raw draw (U[0,1), integer index, or N(0,1)); the kernel applies low+(high-low)*u.
 * mbx_reset (init_population, rlepso_optimizer.py:40-42) uses the reinit_pos_u / reinit_vel_u /
 * noise_reinit slots.  The three noise rows hold the noise model's draws in the reference's call
 * order (gauss: N; uniform: U,U'; cauchy: U,N,N').                                                    */
#define MBX_RLEPSO_TAPE_RAND1(NP, D)      ((int64_t)0)
#define MBX_RLEPSO_TAPE_RAND2(NP, D)      ((int64_t)(NP))
#define MBX_RLEPSO_TAPE_CLPSO(NP, D)      ((int64_t)2 * (NP))
#define MBX_RLEPSO_TAPE_TOURN(NP, D)      ((int64_t)2 * (NP) + (int64_t)(NP) * (D))
#define MBX_RLEPSO_TAPE_FDR(NP, D)        ((int64_t)2 * (NP) + (int64_t)3 * (NP) * (D))
#define MBX_RLEPSO_TAPE_NOISE0(NP, D)     ((int64_t)2 * (NP) + (int64_t)4 * (NP) * (D))
#define MBX_RLEPSO_TAPE_REINIT(NP, D)     ((int64_t)5 * (NP) + (int64_t)4 * (NP) * (D))
#define MBX_RLEPSO_TAPE_REPOS(NP, D)      ((int64_t)6 * (NP) + (int64_t)4 * (NP) * (D))
#define MBX_RLEPSO_TAPE_REVEL(NP, D)      ((int64_t)6 * (NP) + (int64_t)5 * (NP) * (D))
#define MBX_RLEPSO_TAPE_NOISE1(NP, D)     ((int64_t)6 * (NP) + (int64_t)6 * (NP) * (D))
#define MBX_RLEPSO_TAPE_STRIDE(NP, D)     ((int64_t)9 * (NP) + (int64_t)6 * (NP) * (D))

/* ---------------------------------------------------------------- 2. RLEPSO instance state (HBM, doubles)
 * One contiguous block per instance (one workgroup streams it in and out per generation):
 *   cur_pos[NP*D] vel[NP*D] pbest_pos[NP*D] c_cost[NP] pbest[NP] per_no_improve[NP] gbest_pos[D]
 *   scalars[MBX_NSCALAR] cost_curve[n_logpoint+1]
 * (the fields of RLEPSO_Optimizer.__particles, rlepso_optimizer.py:53-61, plus fes/cost/log_index).   */
#define MBX_RLEPSO_ST_POS(NP, D)      ((int64_t)0)
#define MBX_RLEPSO_ST_VEL(NP, D)      ((int64_t)(NP) * (D))
#define MBX_RLEPSO_ST_PBPOS(NP, D)    ((int64_t)2 * (NP) * (D))
#define MBX_RLEPSO_ST_CCOST(NP, D)    ((int64_t)3 * (NP) * (D))
#define MBX_RLEPSO_ST_PBEST(NP, D)    ((int64_t)3 * (NP) * (D) + (NP))
#define MBX_RLEPSO_ST_PNI(NP, D)      ((int64_t)3 * (NP) * (D) + 2 * (NP))
#define MBX_RLEPSO_ST_GBPOS(NP, D)    ((int64_t)3 * (NP) * (D) + 3 * (NP))
#define MBX_RLEPSO_ST_SCALARS(NP, D)  ((int64_t)3 * (NP) * (D) + 3 * (NP) + (D))

/* scalar slots (shared by every algorithm's state block) */
#define MBX_SC_GBEST      0   /* gbest_val                                         */
#define MBX_SC_FES        1   /* optimizer.fes                                     */
#define MBX_SC_LOG_INDEX  2   /* optimizer.log_index                               */
#define MBX_SC_COST_LEN   3   /* len(optimizer.cost)                               */
#define MBX_SC_DONE       4   /* 1.0 once update() has returned is_done            */
#define MBX_SC_RETURN     5   /* sum of rewards (rollout_episode's R)              */
#define MBX_SC_GEN        6   /* number of update() calls executed this episode    */
#define MBX_SC_EPISODE    7   /* number of resets so far (Philox counter word 3)   */
#define MBX_SC_GBEST_IDX  8   /* gbest_index                                       */
#define MBX_SC_REINIT     9   /* 1.0 if __reinit fired in the last step (diagnostic) */
#define MBX_NSCALAR       16

#define MBX_RLEPSO_STATE_DOUBLES(NP, D, NLOG) \
    (MBX_RLEPSO_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)

/* ---------------------------------------------------------------- 3. Philox4x32-10 draw sites
 * key     = (seed_lo, seed_hi)             the instance's 64-bit seed
 * counter = (index, site, generation, episode)
 * A call yields four 32-bit words w0..w3.  u53(a,b) = ((a>>5)*2^26 + (b>>6)) / 2^53  in [0,1).
 * Integer draws in [0,n): mulhi32(w, n).  Normal pairs: Box-Muller on (1-u53(w0,w1), u53(w2,w3)):
 * r = sqrt(-2 ln(1-ua)), n0 = r cos(2 pi ub), n1 = r sin(2 pi ub).
 *
 *   site                 index        words
 *   MBX_SITE_ELEM_A      e >> 1       RLEPSO: ONE call per element pair carries its four element-wise uniforms, 32 bits each, u32(w) = w / 2^32:
 *                                     u32(w0) = clpso_u[e] and u32(w2) = fdr_u[e] for the even element, u32(w1) / u32(w3) for the odd one
 *                                     (the CLPSO mask compares against pci in [0.05, 0.5] and both act as step weights: 2^-32 resolution)
 *   MBX_SITE_TOURN       e >> 1       mulhi(w0,NP), mulhi(w1,NP) = tournament pair of the even element, mulhi(w2,NP), mulhi(w3,NP) = of the odd one;
 *                                     only consumed where !(clpso_u[e] > pci_i)
 *   MBX_SITE_ELEM_B      -            (RLEPSO: not drawn any more; the FDR weights ride in the ELEM_A call)
 *   MBX_SITE_PART        i            u53(w0,w1) = rand1[i];    u53(w2,w3) = rand2[i]
 *   MBX_SITE_REINIT      i            u53(w0,w1) = reinit_u[i]
 *   MBX_SITE_ELEM_R      e            u53(w0,w1) = pos_u[e];    u53(w2,w3) = vel_u[e]   (init + reinit)
 *   MBX_SITE_NOISE0_A/B  i            main evaluation:   A -> (ua,ub), B -> (uc,ud)
 *   MBX_SITE_NOISE1_A/B  i            init / reinit evaluation
 *       gauss  : N = n0(ua,ub)            uniform: U = ua, U' = ub
 *       cauchy : U = ua, (N, N') = (n0, n1)(uc,ud)
 */
#define MBX_SITE_ELEM_A    0u
#define MBX_SITE_ELEM_B    1u
#define MBX_SITE_PART      2u
#define MBX_SITE_REINIT    3u
#define MBX_SITE_ELEM_R    4u
#define MBX_SITE_NOISE0_A  5u
#define MBX_SITE_NOISE0_B  6u
#define MBX_SITE_NOISE1_A  7u
#define MBX_SITE_NOISE1_B  8u
/* stand-alone mbx_eval noise: counter = (row, MBX_SITE_EVAL_A/B, 0, 0) */
#define MBX_SITE_EVAL_A    9u
#define MBX_SITE_EVAL_B    10u

/* ---------------------------------------------------------------- 4. LDE (lde_optimizer.py) layouts
 * tape per step, draw order of LDE_Optimizer.update (:88-90 pbest index, :109-121 r1/r2 after rejection,
 * :44-47 crossover uniforms + jrand, eval noise):
 *   pbest_idx[NP] r0[NP] r1[NP] jrand[NP] noise[3*NP] cross_u[NP*D]
 * mbx_reset (init_population :133-134) uses cross_u as the position uniforms and noise[] for the evaluation.
 * state block: pop[NP*D] (kept sorted by fitness, :74-79) fit[NP] hist_sum[8] scalars[16] cost_curve[nlog+1];
 * hist_sum accumulates past_histo (:139,186), scalars[MBX_SC_HCOUNT] its length.
 * Philox: MBX_SITE_LDE_PART(i): mulhi(w0,bound)=pbest_idx, w1 -> r0 over the NP-1 indices != i, w2 -> r1 over the
 * NP-2 indices not in {i,r0} (same distribution as the reference's rejection loop), mulhi(w3,D)=jrand;
 * MBX_SITE_LDE_ELEM: reset (generation 0), index e: u53(w0,w1) = initial-position uniform;  step (generation >= 1), index e >> 2: ONE call per
 * four consecutive elements, u32(w[e & 3]) = w / 2^32 = crossover uniform of element e (compared against the float32 rate CR_i).               */
#define MBX_LDE_TAPE_PIDX(NP, D)   ((int64_t)0)
#define MBX_LDE_TAPE_R0(NP, D)     ((int64_t)(NP))
#define MBX_LDE_TAPE_R1(NP, D)     ((int64_t)2 * (NP))
#define MBX_LDE_TAPE_JRAND(NP, D)  ((int64_t)3 * (NP))
#define MBX_LDE_TAPE_NOISE(NP, D)  ((int64_t)4 * (NP))
#define MBX_LDE_TAPE_CROSS(NP, D)  ((int64_t)7 * (NP))
#define MBX_LDE_TAPE_STRIDE(NP, D) ((int64_t)7 * (NP) + (int64_t)(NP) * (D))
#define MBX_LDE_BINS 5
#define MBX_LDE_ST_POP(NP, D)      ((int64_t)0)
#define MBX_LDE_ST_FIT(NP, D)      ((int64_t)(NP) * (D))
#define MBX_LDE_ST_HSUM(NP, D)     ((int64_t)(NP) * (D) + (NP))      /* 8 doubles: [0..5) running sum of past_histo, [5] the last histogram, packed 10 bits per bin */
#define MBX_LDE_ST_SCALARS(NP, D)  ((int64_t)(NP) * (D) + (NP) + 8)
#define MBX_LDE_STATE_DOUBLES(NP, D, NLOG) (MBX_LDE_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_HCOUNT 10
#define MBX_SITE_LDE_PART  11u
#define MBX_SITE_LDE_ELEM  12u

/* ---------------------------------------------------------------- 5. DE-DDQN (de_ddqn_optimizer.py) layouts
 * tape per step (draw order of update(): binomial's randint(D,1) and rand(1,D) (operators/crossover.py:11,14), eval
 * noise of the single trial, then __get_state's randint(0,NP,5) (:85)):
 *   r[5] @0 | jrand @5 | noise[3] @8 | cross_u[D] @16
 * mbx_reset: r[5] @0 | pos_u[NP*D] @16 | noise_init[3*NP] @16+NP*D.
 * state block: X[NP*D] cost[NP] gbest_pos[D] prebest_pos[D] r[8] N_tot[4*10] N_succ[4*4*10] OM_sum[4*4*10]
 *   OM_max[4*4*10] OM_W[50*6] extra[16] scalars[16] cost_curve[nlog+1].
 * The generation deques (maxlen gen_max = 10, appendleft) are rings: generation-back index g lives in slot
 * (g - gen) mod 10.  extra[]: see MBX_DQ_X_*.  Philox: MBX_SITE_DQ_R(idx 0: w0..w3 -> r0..r3, idx 1: w0 -> r4),
 * MBX_SITE_DQ_JRAND(idx 0: w0), cross_u -> MBX_SITE_LDE_ELEM(d), init positions -> MBX_SITE_LDE_ELEM(e).        */
#define MBX_DQ_GENMAX 10
#define MBX_DQ_W      50
#define MBX_DQ_NFEAT  99
#define MBX_DQ_TAPE_R(NP, D)       ((int64_t)0)
#define MBX_DQ_TAPE_JRAND(NP, D)   ((int64_t)5)
#define MBX_DQ_TAPE_NOISE(NP, D)   ((int64_t)8)
#define MBX_DQ_TAPE_CROSS(NP, D)   ((int64_t)16)
#define MBX_DQ_TAPE_POS(NP, D)     ((int64_t)16)
#define MBX_DQ_TAPE_NOISE_INIT(NP, D) ((int64_t)16 + (int64_t)(NP) * (D))
#define MBX_DQ_TAPE_STRIDE(NP, D)  ((int64_t)16 + (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_DQ_ST_X(NP, D)        ((int64_t)0)
#define MBX_DQ_ST_COST(NP, D)     ((int64_t)(NP) * (D))
#define MBX_DQ_ST_GBPOS(NP, D)    ((int64_t)(NP) * (D) + (NP))
#define MBX_DQ_ST_PREPOS(NP, D)   (MBX_DQ_ST_GBPOS(NP, D) + (D))
#define MBX_DQ_ST_R(NP, D)        (MBX_DQ_ST_PREPOS(NP, D) + (D))
#define MBX_DQ_ST_NTOT(NP, D)     (MBX_DQ_ST_R(NP, D) + 8)
#define MBX_DQ_ST_NSUCC(NP, D)    (MBX_DQ_ST_NTOT(NP, D) + 40)
#define MBX_DQ_ST_OMSUM(NP, D)    (MBX_DQ_ST_NSUCC(NP, D) + 160)
#define MBX_DQ_ST_OMMAX(NP, D)    (MBX_DQ_ST_OMSUM(NP, D) + 160)
#define MBX_DQ_ST_OMW(NP, D)      (MBX_DQ_ST_OMMAX(NP, D) + 160)
#define MBX_DQ_ST_EXTRA(NP, D)    (MBX_DQ_ST_OMW(NP, D) + 300)
#define MBX_DQ_ST_SCALARS(NP, D)  (MBX_DQ_ST_EXTRA(NP, D) + 16)
#define MBX_DQ_STATE_DOUBLES(NP, D, NLOG) (MBX_DQ_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_DQ_X_GWORST   0   /* c_gworst                                            */
#define MBX_DQ_X_CPRE     1   /* c_prebest (never updated after init: reference :135) */
#define MBX_DQ_X_POINTER  2
#define MBX_DQ_X_GEN      3   /* the reference's __gen (population sweeps started)    */
#define MBX_DQ_X_STAG     4
#define MBX_DQ_X_OMWLEN   5
#define MBX_DQ_X_G0       6   /* row that X_gbest / X_prebest alias while they are numpy views (:55,58) */
#define MBX_DQ_X_GBVIEW   7
#define MBX_DQ_X_PREVIEW  8
#define MBX_DQ_X_MEDLO    9   /* cache: the cost order statistics NP/2 - 1 and NP/2 the last update() found (NaN after reset); */
#define MBX_DQ_X_MEDHI    10  /* the next update() re-validates them with one counting pass before it trusts them          */
#define MBX_SITE_DQ_R      13u
#define MBX_SITE_DQ_JRAND  14u
/* mbx_gauss_policy: index j = action component, u53(w0,w1), u53(w2,w3) -> Box-Muller, first normal used */
#define MBX_SITE_POLICY    15u

/* ---------------------------------------------------------------- 6. Random_search (random_search.py) layouts
 * tape per step / reset: pos_u[NP*D] | noise[3*NP];  state block: scalars[16] cost_curve[nlog+1].
 * Philox: positions MBX_SITE_LDE_ELEM(e), noise MBX_SITE_NOISE0_A/B(i), generation counter = number of populations
 * drawn so far in the episode (0 for the initial one).                                                              */
#define MBX_RS_TAPE_POS(NP, D)     ((int64_t)0)
#define MBX_RS_TAPE_NOISE(NP, D)   ((int64_t)(NP) * (D))
#define MBX_RS_TAPE_STRIDE(NP, D)  ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_RS_ST_SCALARS(NP, D)   ((int64_t)0)
#define MBX_RS_STATE_DOUBLES(NP, D, NLOG) ((int64_t)MBX_NSCALAR + (int64_t)(NLOG) + 1)

/* ---------------------------------------------------------------- 7. RL-PSO (rl_pso_optimizer.py) layouts
 * One env step = ONE particle (index `cur`, round robin): velocity / position update with the action as the gbest
 * attraction weight, one evaluation, pbest / gbest, reward (pre_cost - new_cost) / (max_cost - gbest) (:76-148).
 * state vector [2 D] = gbest_position | current_position[cur]  (:62-63);  action [1] float32.
 * state block: pos[NP*D] vel[NP*D] pbest_pos[NP*D] c_cost[NP] pbest[NP] gbest_pos[D] scalars[16] cost_curve[nlog+1];
 * scalars beyond the common ones: inertia w (decremented EVERY step, :85-86), max_cost of the initial population (:41),
 * cur.  tape per reset: pos_u[NP*D] | vel_u[NP*D] | noise[3*NP] (draw order of init_population :30-36);
 * tape per step: rand1 | noise[3] (:89, then the evaluation's own draws).
 * Philox: reset (gen 0): MBX_SITE_ELEM_R(e): u53(w0,w1) = pos_u, u53(w2,w3) = vel_u; noise MBX_SITE_NOISE1_A/B(i).
 *         step (gen = number of the step): MBX_SITE_PART(0): u53(w0,w1) = rand1; noise MBX_SITE_NOISE0_A/B(0).       */
#define MBX_RLPSO_TAPE_POS(NP, D)    ((int64_t)0)
#define MBX_RLPSO_TAPE_VEL(NP, D)    ((int64_t)(NP) * (D))
#define MBX_RLPSO_TAPE_NOISE_INIT(NP, D) (2 * (int64_t)(NP) * (D))
#define MBX_RLPSO_TAPE_RAND1(NP, D)  ((int64_t)0)
#define MBX_RLPSO_TAPE_NOISE(NP, D)  ((int64_t)1)
#define MBX_RLPSO_TAPE_STRIDE(NP, D) (2 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_RLPSO_ST_POS(NP, D)      ((int64_t)0)
#define MBX_RLPSO_ST_VEL(NP, D)      ((int64_t)(NP) * (D))
#define MBX_RLPSO_ST_PBPOS(NP, D)    (2 * (int64_t)(NP) * (D))
#define MBX_RLPSO_ST_CCOST(NP, D)    (3 * (int64_t)(NP) * (D))
#define MBX_RLPSO_ST_PBEST(NP, D)    (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_RLPSO_ST_GBPOS(NP, D)    (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_RLPSO_ST_SCALARS(NP, D)  (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP) + (D))
#define MBX_RLPSO_STATE_DOUBLES(NP, D, NLOG) (MBX_RLPSO_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_RLPSO_W       10
#define MBX_SC_RLPSO_MAXCOST 11
#define MBX_SC_RLPSO_CUR     12

/* ---------------------------------------------------------------- 8. GLEET (gleet_optimizer.py) layouts
 * One env step = one PSO generation; action [NP] float32 = each particle's share of the pbest attraction (:206-210);
 * state [NP, 27] = 9 features of the particle (observe() :127-152) | the features it had when it last improved
 * (pbest_feature) | the features of the gbest particle when gbest last improved (gbest_feature)  (:111-124, 290-296).
 * state block: pos[NP*D] vel[NP*D] pbest_pos[NP*D] c_cost[NP] pbest[NP] per_no_improve[NP] gbest_pos[D]
 *              pbest_feature[NP*9] gbest_feature[9 (+1 pad)] scalars[16] cost_curve[nlog+1];
 * scalars beyond the common ones: inertia w (-= 0.5 / (maxFEs / NP) per generation), max_cost (= the MINIMUM of the initial
 * costs, :51), no_improve.
 * tape per reset: pos_u[NP*D] | vel_u[NP*D] | noise[3*NP];  per step: rand1[NP] | rand2[NP] | noise[3*NP].
 * Philox: reset (gen 0): MBX_SITE_ELEM_R(e): u53(w0,w1) = pos_u, u53(w2,w3) = vel_u; noise MBX_SITE_NOISE1_A/B(i).
 *         step (gen = generation): MBX_SITE_PART(i): u53(w0,w1) = rand1, u53(w2,w3) = rand2; noise MBX_SITE_NOISE0_A/B(i). */
#define MBX_GLEET_NFEAT 9
#define MBX_GLEET_TAPE_POS(NP, D)    ((int64_t)0)
#define MBX_GLEET_TAPE_VEL(NP, D)    ((int64_t)(NP) * (D))
#define MBX_GLEET_TAPE_NOISE_INIT(NP, D) (2 * (int64_t)(NP) * (D))
#define MBX_GLEET_TAPE_RAND1(NP, D)  ((int64_t)0)
#define MBX_GLEET_TAPE_RAND2(NP, D)  ((int64_t)(NP))
#define MBX_GLEET_TAPE_NOISE(NP, D)  (2 * (int64_t)(NP))
#define MBX_GLEET_TAPE_STRIDE(NP, D) (2 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_GLEET_ST_POS(NP, D)      ((int64_t)0)
#define MBX_GLEET_ST_VEL(NP, D)      ((int64_t)(NP) * (D))
#define MBX_GLEET_ST_PBPOS(NP, D)    (2 * (int64_t)(NP) * (D))
#define MBX_GLEET_ST_CCOST(NP, D)    (3 * (int64_t)(NP) * (D))
#define MBX_GLEET_ST_PBEST(NP, D)    (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_GLEET_ST_PNI(NP, D)      (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_GLEET_ST_GBPOS(NP, D)    (3 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_GLEET_ST_PFEAT(NP, D)    (3 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP) + (D))
#define MBX_GLEET_ST_GFEAT(NP, D)    (MBX_GLEET_ST_PFEAT(NP, D) + 9 * (int64_t)(NP))
#define MBX_GLEET_ST_SCALARS(NP, D)  (MBX_GLEET_ST_GFEAT(NP, D) + 10)
#define MBX_GLEET_STATE_DOUBLES(NP, D, NLOG) (MBX_GLEET_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_GLEET_W         10
#define MBX_SC_GLEET_MAXCOST   11
#define MBX_SC_GLEET_NOIMPROVE 12

/* ---------------------------------------------------------------- 9. QLPSO (qlpso_optimizer.py) layouts
 * One env step = ONE particle (round robin over NP = 30): ring-neighbourhood best of size 4 / 8 / 16 / 30 chosen by the action,
 * velocity (W = 0.729844, C = 1.49618, no velocity clamp), position clipping, one evaluation, swarm diversity, reward in
 * {2, 1, 0, -2} from (cost improved?, diversity grew?) (:7-16, 45-125).  state [1] = the action the NEXT particle took last time
 * (initially a random integer in 0..3, :89); action [1] int32 in 0..3.  The pointer is NOT reset by init_population (:33).
 * state block: pop[NP*D] vel[NP*D] pbest_pos[NP*D] cost[NP] sstate[NP] scalars[16] cost_curve[nlog+1];
 * scalars beyond the common ones: diversity, pointer.
 * tape per reset: pos_u[NP*D] | noise[3*NP] | sstate[NP];  per step: rand_a | rand_b | noise[3] | choice_u (the uniform that
 * QLPSO_Agent's np.random.choice consumes before the step; used by the fused policy only).
 * Philox: reset (gen 0): MBX_SITE_LDE_ELEM(e): u53(w0,w1) = pos_u; noise MBX_SITE_NOISE1_A/B(i); MBX_SITE_PART(i): mulhi(w0, 4) = sstate.
 *         step (gen = number of the step): MBX_SITE_PART(0): u53(w0,w1) = rand_a, u53(w2,w3) = rand_b; noise MBX_SITE_NOISE0_A/B(0);
 *         MBX_SITE_POLICY(0): u53(w0,w1) = choice_u.                                                                              */
#define MBX_QLPSO_TAPE_POS(NP, D)        ((int64_t)0)
#define MBX_QLPSO_TAPE_NOISE_INIT(NP, D) ((int64_t)(NP) * (D))
#define MBX_QLPSO_TAPE_SSTATE(NP, D)     ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_QLPSO_TAPE_RAND(NP, D)       ((int64_t)0)
#define MBX_QLPSO_TAPE_NOISE(NP, D)      ((int64_t)2)
#define MBX_QLPSO_TAPE_CHOICE(NP, D)     ((int64_t)5)
#define MBX_QLPSO_TAPE_STRIDE(NP, D)     ((int64_t)(NP) * (D) + 4 * (int64_t)(NP) + 8)
#define MBX_QLPSO_ST_POP(NP, D)          ((int64_t)0)
#define MBX_QLPSO_ST_VEL(NP, D)          ((int64_t)(NP) * (D))
#define MBX_QLPSO_ST_PBPOS(NP, D)        (2 * (int64_t)(NP) * (D))
#define MBX_QLPSO_ST_COST(NP, D)         (3 * (int64_t)(NP) * (D))
#define MBX_QLPSO_ST_SSTATE(NP, D)       (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_QLPSO_ST_SCALARS(NP, D)      (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_QLPSO_STATE_DOUBLES(NP, D, NLOG) (MBX_QLPSO_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_QLPSO_DIVERSITY 10
#define MBX_SC_QLPSO_POINTER   11

/* ---------------------------------------------------------------- 10. classic baselines (deap_de.py, deap_pso.py, deap_cmaes.py)
 * No agent: mbx_reset builds and evaluates the initial population, every mbx_step (actions = NULL) is one sweep over the
 * population (DE, PSO: NP sequential single-individual updates, each billed 1 FE and checked for logging / termination like the
 * reference's inner loop) or one generation (CMA-ES).  state [1] = fes / maxFEs.  DEAP itself (deap==1.3.3, requirements.txt:7) is
 * not part of the reference tree: DE and PSO are fully written out in the reference's wrappers, CMA-ES follows deap.cma.Strategy's
 * published algorithm.  There are no reference traces for these (parity unpinned); no replay tape either.
 * DE   (deap_de.py:8-82, NP 50, F 0.5, Cr 0.5, selTournament(k=3, tournsize=3) donors):
 *      state block: X[NP*D] cost[NP] scalars[16] cost_curve[nlog+1].
 *      Philox, reset (gen 0): MBX_SITE_LDE_ELEM(e) -> position; noise MBX_SITE_NOISE1_A/B(i).
 *      sweep (gen = sweep number): MBX_SITE_CLASSIC(3k+j), j = 0..2: mulhi(w0..w2, NP) = the three aspirants of donor j,
 *      w3 of j = 0: mulhi(w3, D) = forced crossover index; MBX_SITE_LDE_ELEM(k*D+i) -> crossover uniform; noise MBX_SITE_NOISE0_A/B(k).
 * PSO  (deap_pso.py:8-122, 50 particles, phi1 = phi2 = 2, speed in +-ub/2, gbest updated inside the sweep):
 *      state block: X[NP*D] speed[NP*D] pbest_pos[NP*D] pbest[NP] gbest_pos[D] scalars[16] cost_curve[nlog+1].
 *      Philox, reset: MBX_SITE_ELEM_R(e): u53(w0,w1) -> position, u53(w2,w3) -> speed; noise MBX_SITE_NOISE1_A/B(i).
 *      sweep: MBX_SITE_ELEM_A(k*D+i): u53(w0,w1) -> u1, u53(w2,w3) -> u2; noise MBX_SITE_NOISE0_A/B(k).
 * CMAES (deap_cmaes.py:12-66 + deap.cma.Strategy, lambda 50, centroid = ub, sigma 0.5):
 *      state block: centroid[D] C[D*D] B[D*D] diagD[D] ps[D] pc[D] scalars[16] cost_curve[nlog+1]; scalars: sigma, update_count.
 *      Philox, generation g >= 1: MBX_SITE_ELEM_A(i*D+d): Box-Muller(u53(w0,w1), u53(w2,w3)) first normal -> arz[i][d];
 *      noise MBX_SITE_NOISE0_A/B(i).                                                                                            */
#define MBX_SITE_CLASSIC     16u
#define MBX_SITE_TOURN       17u   /* RLEPSO, see the table above */
#define MBX_DE_ST_X(NP, D)          ((int64_t)0)
#define MBX_DE_ST_COST(NP, D)       ((int64_t)(NP) * (D))
#define MBX_DE_ST_SCALARS(NP, D)    ((int64_t)(NP) * (D) + (NP))
#define MBX_DE_STATE_DOUBLES(NP, D, NLOG) (MBX_DE_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_PSO_ST_X(NP, D)         ((int64_t)0)
#define MBX_PSO_ST_SPEED(NP, D)     ((int64_t)(NP) * (D))
#define MBX_PSO_ST_PBPOS(NP, D)     (2 * (int64_t)(NP) * (D))
#define MBX_PSO_ST_PBEST(NP, D)     (3 * (int64_t)(NP) * (D))
#define MBX_PSO_ST_GBPOS(NP, D)     (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_PSO_ST_SCALARS(NP, D)   (3 * (int64_t)(NP) * (D) + (NP) + (D))
#define MBX_PSO_STATE_DOUBLES(NP, D, NLOG) (MBX_PSO_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_CMA_ST_CENTROID(NP, D)  ((int64_t)0)
#define MBX_CMA_ST_C(NP, D)         ((int64_t)(D))
#define MBX_CMA_ST_B(NP, D)         ((int64_t)(D) + (int64_t)(D) * (D))
#define MBX_CMA_ST_DIAGD(NP, D)     ((int64_t)(D) + 2 * (int64_t)(D) * (D))
#define MBX_CMA_ST_PS(NP, D)        (2 * (int64_t)(D) + 2 * (int64_t)(D) * (D))
#define MBX_CMA_ST_PC(NP, D)        (3 * (int64_t)(D) + 2 * (int64_t)(D) * (D))
#define MBX_CMA_ST_SCALARS(NP, D)   (4 * (int64_t)(D) + 2 * (int64_t)(D) * (D))
#define MBX_CMA_STATE_DOUBLES(NP, D, NLOG) (MBX_CMA_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_CMA_SIGMA   10
#define MBX_SC_CMA_UPDATES 11

/* ---------------------------------------------------------------- 11. GL-PSO (gl_pso.py) layouts
 * No agent: mbx_reset is init_population (:76-107: random swarm, one evaluation, then one exemplar update with init = True -- 2 NP FEs),
 * every mbx_step (actions = NULL) is one __update (:118-177: velocity / position, evaluation, pbest / gbest, logging, exemplar update,
 * termination -- 2 NP FEs).  NP 100, pm 0.01, nsel 10, w 0.7298, c1 1.49618, sg 7, velocity cap 0.2 (ub - lb).  state [1] = fes / maxFEs.
 * state block: X[NP*D] V[NP*D] pbest_pos[NP*D] pbest[NP] exemplar[NP*D] exemplar_cost[NP] stag[NP] gbest_pos[D] scalars[16] cost_curve[nlog+1].
 * stag (exemplar_stag) lives on the reference's optimizer object and is never reset by init_population: mbx_reset leaves it alone, so a
 * batch carries it from episode to episode (mbx_batch_rebind included); a new batch starts at zero.
 * tape per reset: pos_u[NP*D] | vel_u[NP*D] | noise[3*NP] | <exemplar block>
 * tape per step:  rand[NP*D] | noise[3*NP] | <exemplar block>
 *   exemplar block (:22-66): cross_idx[NP*D] | cross_u[NP*D] | mut_u[NP*D] | mut_test_u[NP*D] | noise[3*NP] | tour_idx[NP*10]
 *   (randint values stored as doubles; tour_idx is read only when some stag > sg, i.e. when the reference draws it).
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the step:
 *   MBX_SITE_ELEM_R(e)       reset: u53(w0,w1) = pos_u, u53(w2,w3) = vel_u
 *   MBX_SITE_ELEM_A(e)       step:  u53(w0,w1) = rand
 *   MBX_SITE_NOISE1_A/B(i)   reset: evaluation of the swarm        MBX_SITE_NOISE0_A/B(i)  step: evaluation of the swarm
 *   MBX_SITE_GL_CROSS(e)     mulhi(w0, NP) = cross_idx, u53(w2,w3) = cross_u
 *   MBX_SITE_GL_MUT(e)       u53(w0,w1) = mut_u, u53(w2,w3) = mut_test_u
 *   MBX_SITE_GL_NOISE_A/B(i) evaluation of the new exemplars (reset and step)
 *   MBX_SITE_GL_TOUR(i*10+j) mulhi(w0, NP) = tour_idx[i][j]                                                                            */
#define MBX_GLPSO_NSEL 10
#define MBX_GLPSO_TAPE_POS(NP, D)        ((int64_t)0)
#define MBX_GLPSO_TAPE_VEL(NP, D)        ((int64_t)(NP) * (D))
#define MBX_GLPSO_TAPE_NOISE_INIT(NP, D) (2 * (int64_t)(NP) * (D))
#define MBX_GLPSO_TAPE_XB_INIT(NP, D)    (2 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_GLPSO_TAPE_RAND(NP, D)       ((int64_t)0)
#define MBX_GLPSO_TAPE_NOISE(NP, D)      ((int64_t)(NP) * (D))
#define MBX_GLPSO_TAPE_XB(NP, D)         ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
/* offsets inside the exemplar block */
#define MBX_GLPSO_XB_CIDX(NP, D)         ((int64_t)0)
#define MBX_GLPSO_XB_CU(NP, D)           ((int64_t)(NP) * (D))
#define MBX_GLPSO_XB_MU(NP, D)           (2 * (int64_t)(NP) * (D))
#define MBX_GLPSO_XB_MTEST(NP, D)        (3 * (int64_t)(NP) * (D))
#define MBX_GLPSO_XB_NOISE(NP, D)        (4 * (int64_t)(NP) * (D))
#define MBX_GLPSO_XB_TOUR(NP, D)         (4 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_GLPSO_TAPE_STRIDE(NP, D)     (6 * (int64_t)(NP) * (D) + 6 * (int64_t)(NP) + (int64_t)MBX_GLPSO_NSEL * (NP))
#define MBX_GLPSO_ST_X(NP, D)            ((int64_t)0)
#define MBX_GLPSO_ST_V(NP, D)            ((int64_t)(NP) * (D))
#define MBX_GLPSO_ST_PBPOS(NP, D)        (2 * (int64_t)(NP) * (D))
#define MBX_GLPSO_ST_PBEST(NP, D)        (3 * (int64_t)(NP) * (D))
#define MBX_GLPSO_ST_EX(NP, D)           (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_GLPSO_ST_EXCOST(NP, D)       (4 * (int64_t)(NP) * (D) + (NP))
#define MBX_GLPSO_ST_STAG(NP, D)         (4 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_GLPSO_ST_GBPOS(NP, D)        (4 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_GLPSO_ST_SCALARS(NP, D)      (4 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP) + (D))
#define MBX_GLPSO_STATE_DOUBLES(NP, D, NLOG) (MBX_GLPSO_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SITE_GL_CROSS    18u
#define MBX_SITE_GL_MUT      19u
#define MBX_SITE_GL_NOISE_A  20u
#define MBX_SITE_GL_NOISE_B  21u
#define MBX_SITE_GL_TOUR     22u

/* ---------------------------------------------------------------- 12. JDE21 (jde21.py) layouts
 * No agent: mbx_reset is __init_population (:68-81: NP = 170 random rows, one evaluation, F = 0.5, Cr = 0.9 -- 170 FEs), every mbx_step
 * (actions = NULL) is one __update (:83-265): a big-population pass of bNP trials with crowding, then bNP / 10 small-population passes of 10
 * trials -- 2 bNP FEs; bNP = 160 halves up to three times.  cfg.np must be 170.  state [1] = fes / maxFEs.
 * state block: pop[NP*D] cost[NP] F[NP] Cr[NP] crowd[NP] scalars[16] cost_curve[nlog+1].  Rows [0, bNP) are the big population, rows
 * [bNP, bNP + 10) the small one, rows beyond are dead after a halving.  crowd[i], i < bNP: the crowding target of trial i in the last step
 * (diagnostic).  scalars beyond the common ones: bNP, cbest, cbest_id and the counters nReset / sReset / cCopy (zeroed by mbx_reset).
 * A step has R = 2 (NP - 10) = 320 trial rows: row i < 160 is trial i of the big pass, row 160 + 10 p + i trial i of small pass p.
 * tape per reset: pos_u[NP*D] | noise[3*NP]
 * tape per step (per-row slots are [R] each; index values are the RESOLVED ones, after the reference's rejection loops, as doubles; the
 *   small passes' indices are absolute rows bNP + k):
 *   r1 | r2 | r3 | randF_u | randCr_u | rvsF | rvsCr | jrand | noise[3*R] | cross_u[R*D] | reseed_big_u[(NP-10)*D] | reseed_small_u[10*D]
 *   (the kernel applies u * Fu + Fl etc.; reseed_* are read only when the reset branch fires, i.e. when the reference draws them).
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the step; t = trial row:
 *   MBX_SITE_JD_IDX(t*32+a)  attempt a = 0..25 of the bounded redraw: mulhi(w0, n) = r1, mulhi(w1, n') = r2, mulhi(w2, n') = r3, each with
 *                            its own attempt counter (a draw is redrawn while the reference's test rejects it, 25 times at most, and
 *                            then kept); a = 0: mulhi(w3, D) = jrand
 *   MBX_SITE_JD_PART(t)      u53(w0,w1) = randF_u, u53(w2,w3) = randCr_u        MBX_SITE_JD_PART2(t)  u53(w0,w1) = rvsF, u53(w2,w3) = rvsCr
 *   MBX_SITE_JD_CROSS(t*D+d) u53(w0,w1) = cross_u;  reset: index e, u53(w0,w1) = pos_u
 *   MBX_SITE_JD_RESEED(e)    u53(w0,w1) = reseed_big_u[e], u53(w2,w3) = reseed_small_u[e]
 *   MBX_SITE_JD_NOISE_A/B(t) evaluation of trial row t;  reset: MBX_SITE_NOISE1_A/B(i)                                                      */
#define MBX_JDE21_NP   170
#define MBX_JDE21_SNP  10
#define MBX_JDE21_ROWS(NP)               (2 * ((int64_t)(NP) - MBX_JDE21_SNP))
#define MBX_JDE21_TAPE_POS(NP, D)        ((int64_t)0)
#define MBX_JDE21_TAPE_NOISE_INIT(NP, D) ((int64_t)(NP) * (D))
#define MBX_JDE21_TAPE_R1(NP, D)         ((int64_t)0)
#define MBX_JDE21_TAPE_R2(NP, D)         (MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_R3(NP, D)         (2 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_RANDF(NP, D)      (3 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_RANDCR(NP, D)     (4 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_RVSF(NP, D)       (5 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_RVSCR(NP, D)      (6 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_JRAND(NP, D)      (7 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_NOISE(NP, D)      (8 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_CROSS(NP, D)      (11 * MBX_JDE21_ROWS(NP))
#define MBX_JDE21_TAPE_RESEED_B(NP, D)   (11 * MBX_JDE21_ROWS(NP) + MBX_JDE21_ROWS(NP) * (D))
#define MBX_JDE21_TAPE_RESEED_S(NP, D)   (MBX_JDE21_TAPE_RESEED_B(NP, D) + ((int64_t)(NP) - MBX_JDE21_SNP) * (D))
#define MBX_JDE21_TAPE_STRIDE(NP, D)     (MBX_JDE21_TAPE_RESEED_S(NP, D) + (int64_t)MBX_JDE21_SNP * (D))
#define MBX_JDE21_ST_POP(NP, D)          ((int64_t)0)
#define MBX_JDE21_ST_COST(NP, D)         ((int64_t)(NP) * (D))
#define MBX_JDE21_ST_F(NP, D)            ((int64_t)(NP) * (D) + (NP))
#define MBX_JDE21_ST_CR(NP, D)           ((int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_JDE21_ST_CROWD(NP, D)        ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_JDE21_ST_SCALARS(NP, D)      ((int64_t)(NP) * (D) + 4 * (int64_t)(NP))
#define MBX_JDE21_STATE_DOUBLES(NP, D, NLOG) (MBX_JDE21_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_JD_BNP      10
#define MBX_SC_JD_CBEST    11
#define MBX_SC_JD_CBEST_ID 12
#define MBX_SC_JD_NRESET   13
#define MBX_SC_JD_SRESET   14
#define MBX_SC_JD_CCOPY    15
#define MBX_SITE_JD_IDX      23u
#define MBX_SITE_JD_PART     24u
#define MBX_SITE_JD_PART2    25u
#define MBX_SITE_JD_CROSS    26u
#define MBX_SITE_JD_RESEED   27u
#define MBX_SITE_JD_NOISE_A  28u
#define MBX_SITE_JD_NOISE_B  29u

/* ---------------------------------------------------------------- 13. MadDE (madde.py) layouts
 * No agent: mbx_reset is __init_population (:179-195: N0 = 2 D^2 random rows, one evaluation, MF = MCr = 0.2, empty archive -- N0 FEs),
 * every mbx_step (actions = NULL) is one __update (:197-272), NP FEs; NP shrinks linearly from N0 to 4, the archive holds at most
 * NA = int(2.3 NP) rows.  cfg.np must be 2 D^2, D <= 40.  state [1] = fes / maxFEs.  A0 = int(2.3 N0), H = 10 D.
 * state block: pop[2][N0*D] cost[N0] archive[A0*D] MF[H] MCr[H] u[N0*D] ncost[N0] F[N0] Cr[N0] z[N0] c[N0] pm[4] scalars[16] cost_curve[nlog+1].
 *   pop: two buffers, scalars[MBX_SC_MD_LIVE] names the live one; its rows [0, NP) are sorted by (cost, row before the sort), i.e. numpy's
 *   kind='stable' order (the reference's introsort is not reproducible among equal keys); the sort runs at the end of reset and of every
 *   update and moves the rows into the other buffer.  cost: the live costs in that order.  u / ncost / F / Cr: trial rows, their costs and
 *   the F / Cr they were made with, of the last update (after reset: the initial rows in draw order and their costs); rows [0, NP before
 *   the update).  z / c: the standard normal / Cauchy variates behind Cr / F of the last update (diagnostic: the Philox route makes them
 *   with the device's log / cos / tan, which the host does not reproduce to the bit; a tape rebuilt from a Philox step takes them from here).  pm[0..2]: strategy probabilities; mbx_reset leaves them alone (the reference sets them in __init__ only), a new batch
 *   starts at 1/3.  scalars beyond the common ones: NP, archive rows, NA, k (memory slot), live buffer.
 * tape per reset: pos_u[N0*D] | noise[3*N0]
 * tape per step, slots of [N0] indexed by the row i of the sorted population (index values as doubles, RESOLVED, i.e. after the
 *   reference's bounded redraws, and LOCAL as the reference draws them: rb a row of pbest / qbest, r1 a rank inside the row's strategy
 *   group, r2 a rank inside the group or, from the group's size on, an archive row):
 *   mem_idx | z | c | choice_u | rb | r1 | r2 | rvs | qpick | jrand | noise[3*N0] | arc_idx[N0] | cross_u[N0*D]
 *   z / c are STANDARD normal / Cauchy variates (the kernel forms MCr + 0.1 z and c 0.1 + MF); qpick is the row of the qBX pool a row with
 *   rvs <= 0.01 crosses with; arc_idx[k] is the archive row that the improved row of rank k overwrites (read for ranks past the appends).
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the step; i = row:
 *   MBX_SITE_MD_PAR(i)       mulhi(w0, H) = mem_idx, mulhi(w1, pool) = qpick, mulhi(w2, D) = jrand, w3 / 2^32 = rvs
 *   MBX_SITE_MD_NORM(i)      Box-Muller of u53(w0,w1), u53(w2,w3): the cosine half = z
 *   MBX_SITE_MD_CAUCHY(i)    tan(pi (u53(w0,w1) - 0.5)) = c, u53(w2,w3) = choice_u
 *   MBX_SITE_MD_IDX(i*32+a)  attempt a = 0..25 of the bounded redraw: mulhi(w0, n_b) = rb, mulhi(w1, n) = r1, mulhi(w2, n') = r2, each with
 *                            its own attempt counter
 *   MBX_SITE_MD_CROSS(i*D+d) u53(w0,w1) = cross_u;  reset: index e, u53(w0,w1) = pos_u
 *   MBX_SITE_MD_ARC(k)       mulhi(w0, archive rows) = arc_idx[k]
 *   MBX_SITE_MD_NOISE_A/B(i) evaluation of trial row i;  reset: MBX_SITE_NOISE1_A/B(i)                                                      */
#define MBX_MADDE_NP(D)                  (2 * (D) * (D))
#define MBX_MADDE_DIM_MAX                40
#define MBX_MADDE_ARC(NP)                ((int64_t)(2.3 * (double)(NP)))
#define MBX_MADDE_H(D)                   (10 * (int64_t)(D))
#define MBX_MADDE_TAPE_POS(NP, D)        ((int64_t)0)
#define MBX_MADDE_TAPE_NOISE_INIT(NP, D) ((int64_t)(NP) * (D))
#define MBX_MADDE_TAPE_MEM(NP, D)        ((int64_t)0)
#define MBX_MADDE_TAPE_Z(NP, D)          ((int64_t)(NP))
#define MBX_MADDE_TAPE_C(NP, D)          (2 * (int64_t)(NP))
#define MBX_MADDE_TAPE_CHOICE(NP, D)     (3 * (int64_t)(NP))
#define MBX_MADDE_TAPE_RB(NP, D)         (4 * (int64_t)(NP))
#define MBX_MADDE_TAPE_R1(NP, D)         (5 * (int64_t)(NP))
#define MBX_MADDE_TAPE_R2(NP, D)         (6 * (int64_t)(NP))
#define MBX_MADDE_TAPE_RVS(NP, D)        (7 * (int64_t)(NP))
#define MBX_MADDE_TAPE_QPICK(NP, D)      (8 * (int64_t)(NP))
#define MBX_MADDE_TAPE_JRAND(NP, D)      (9 * (int64_t)(NP))
#define MBX_MADDE_TAPE_NOISE(NP, D)      (10 * (int64_t)(NP))
#define MBX_MADDE_TAPE_ARC(NP, D)        (13 * (int64_t)(NP))
#define MBX_MADDE_TAPE_CROSS(NP, D)      (14 * (int64_t)(NP))
#define MBX_MADDE_TAPE_STRIDE(NP, D)     (14 * (int64_t)(NP) + (int64_t)(NP) * (D))
#define MBX_MADDE_ST_POP(NP, D)          ((int64_t)0)
#define MBX_MADDE_ST_COST(NP, D)         (2 * (int64_t)(NP) * (D))
#define MBX_MADDE_ST_ARC(NP, D)          (MBX_MADDE_ST_COST(NP, D) + (NP))
#define MBX_MADDE_ST_MF(NP, D)           (MBX_MADDE_ST_ARC(NP, D) + MBX_MADDE_ARC(NP) * (D))
#define MBX_MADDE_ST_MCR(NP, D)          (MBX_MADDE_ST_MF(NP, D) + MBX_MADDE_H(D))
#define MBX_MADDE_ST_U(NP, D)            (MBX_MADDE_ST_MCR(NP, D) + MBX_MADDE_H(D))
#define MBX_MADDE_ST_NCOST(NP, D)        (MBX_MADDE_ST_U(NP, D) + (int64_t)(NP) * (D))
#define MBX_MADDE_ST_F(NP, D)            (MBX_MADDE_ST_NCOST(NP, D) + (NP))
#define MBX_MADDE_ST_CR(NP, D)           (MBX_MADDE_ST_F(NP, D) + (NP))
#define MBX_MADDE_ST_Z(NP, D)            (MBX_MADDE_ST_CR(NP, D) + (NP))
#define MBX_MADDE_ST_C(NP, D)            (MBX_MADDE_ST_Z(NP, D) + (NP))
#define MBX_MADDE_ST_PM(NP, D)           (MBX_MADDE_ST_C(NP, D) + (NP))
#define MBX_MADDE_ST_SCALARS(NP, D)      (MBX_MADDE_ST_PM(NP, D) + 4)
#define MBX_MADDE_STATE_DOUBLES(NP, D, NLOG) (MBX_MADDE_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_MD_NP       10
#define MBX_SC_MD_ARC      11
#define MBX_SC_MD_NA       12
#define MBX_SC_MD_K        13
#define MBX_SC_MD_LIVE     14
#define MBX_SITE_MD_PAR      30u
#define MBX_SITE_MD_NORM     31u
#define MBX_SITE_MD_CAUCHY   32u
#define MBX_SITE_MD_IDX      33u
#define MBX_SITE_MD_CROSS    34u
#define MBX_SITE_MD_ARC      35u
#define MBX_SITE_MD_NOISE_A  36u
#define MBX_SITE_MD_NOISE_B  37u

/* ---------------------------------------------------------------- 14. DEDQN (dedqn_optimizer.py) layouts
 * One env step = ONE trial vector of the row `pointer` (round robin over NP = 100; the pointer is NOT reset by init_population, :118), built by
 * rand_1_single / cur_to_rand_1_single / best_2_single (action 0 / 1 / anything else; F = 0.5), clipped, binomial crossover (Cr = 0.5), one
 * evaluation, selection `u_cost <= cost[pointer]` -- and then __cal_feature (:130-142): the whole population is evaluated again and its costs
 * are paired BY INDEX with a random walk of rwsteps = NP points through the population's bounding box.  A step bills 2 NP evaluations
 * (:178, :141), a reset 2 NP as well (:153).  state [4] = fdc | rie | acf | nop (:8-76); action [1] int32; reward = cal_reward(survival) (:92-100).
 * state block: pop[NP*D] cost[NP] survival[NP] scost[NP] gbest_pos[D] feat[16] scalars[16] cost_curve[nlog+1].
 *   scost:     the samples_cost of the last __cal_feature (never written back to cost, :133-135).
 *   gbest_pos: the best position once it is an array of its own; while MBX_SC_DEDQN_ALIAS is 1 gbest is still the numpy VIEW of row
 *              MBX_SC_DEDQN_G0 taken by init_population (:151) and follows that row (an equal-cost trial overwrites it, :179-185).
 *   feat:      the four features, then the diagnostics MBX_DEDQN_FEAT_*: the ruggedness level whose entropy is the maximum (first one) and
 *              its six transition counts (:36-47, before the zero counts are replaced), the cost of the last trial, and the three Q values
 *              behind the last action of the in-kernel policy (0 after mbx_step).
 * tape per reset: pos_u[NP*D] | noise_init[3*NP] | walk_u[NP*D] | noise_feat[3*NP]
 * tape per step:  r[4] | jrand | noise_trial[3] | cross_u[D] | walk_u[NP*D] | noise_feat[3*NP]
 *   r: the ACCEPTED row of generate_random_int_single (operators/mutate.py:5-9; 3 columns for actions 0 / 1, 4 otherwise), as doubles;
 *   walk_u[i*D+d]: the uniform of walk step i, coordinate d (random_walk_sampling :79-89).
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the step:
 *   MBX_SITE_LDE_ELEM(e)      reset: u53(w0,w1) = pos_u;  step, index d: u53(w0,w1) = cross_u
 *   MBX_SITE_DD_NOISE_A/B(i)  reset: evaluation of the initial population
 *   MBX_SITE_DD_R(a)          attempt a = 0, 1, ... of the redraw: mulhi(w0..w3, NP) = r[0..3]; all columns are redrawn while the pointer is
 *                             among the columns in use (1024 attempts at most, then kept)
 *   MBX_SITE_DQ_JRAND(0)      mulhi(w0, D) = jrand
 *   MBX_SITE_NOISE0_A/B(0)    evaluation of the trial
 *   MBX_SITE_DD_WALK(i*D+d)   u53(w0,w1) = walk_u
 *   MBX_SITE_NOISE1_A/B(i)    __cal_feature's evaluation of row i (reset and step)                                                       */
#define MBX_DEDQN_NP_MAX   128
#define MBX_DEDQN_DIM_MAX  40
#define MBX_DEDQN_NFEAT    4
#define MBX_DEDQN_TAPE_POS(NP, D)         ((int64_t)0)
#define MBX_DEDQN_TAPE_NOISE_INIT(NP, D)  ((int64_t)(NP) * (D))
#define MBX_DEDQN_TAPE_WALK_INIT(NP, D)   ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_DEDQN_TAPE_NOISE_FEAT0(NP, D) (2 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_DEDQN_TAPE_R(NP, D)           ((int64_t)0)
#define MBX_DEDQN_TAPE_JRAND(NP, D)       ((int64_t)4)
#define MBX_DEDQN_TAPE_NOISE(NP, D)       ((int64_t)5)
#define MBX_DEDQN_TAPE_CROSS(NP, D)       ((int64_t)8)
#define MBX_DEDQN_TAPE_WALK(NP, D)        ((int64_t)8 + (D))
#define MBX_DEDQN_TAPE_NOISE_FEAT(NP, D)  ((int64_t)8 + (D) + (int64_t)(NP) * (D))
#define MBX_DEDQN_TAPE_STRIDE(NP, D)      (2 * (int64_t)(NP) * (D) + 6 * (int64_t)(NP) + 8)
#define MBX_DEDQN_ST_POP(NP, D)           ((int64_t)0)
#define MBX_DEDQN_ST_COST(NP, D)          ((int64_t)(NP) * (D))
#define MBX_DEDQN_ST_SURVIVAL(NP, D)      ((int64_t)(NP) * (D) + (NP))
#define MBX_DEDQN_ST_SCOST(NP, D)         ((int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_DEDQN_ST_GBPOS(NP, D)         ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_DEDQN_ST_FEAT(NP, D)          ((int64_t)(NP) * (D) + 3 * (int64_t)(NP) + (D))
#define MBX_DEDQN_FEAT_SLOTS 16
#define MBX_DEDQN_ST_SCALARS(NP, D)       (MBX_DEDQN_ST_FEAT(NP, D) + MBX_DEDQN_FEAT_SLOTS)
#define MBX_DEDQN_STATE_DOUBLES(NP, D, NLOG) (MBX_DEDQN_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_DEDQN_FEAT_LEVEL  4   /* feat[4]: winning ruggedness level 0..8; feat[5..10]: its six transition counts */
#define MBX_DEDQN_FEAT_COUNTS 5
#define MBX_DEDQN_FEAT_UCOST  11  /* feat[11]: u_cost of the last update() */
#define MBX_DEDQN_FEAT_Q      12  /* feat[12..14]: Q(state) of the last in-kernel decision */
#define MBX_SC_DEDQN_POINTER 10
#define MBX_SC_DEDQN_G0      11
#define MBX_SC_DEDQN_ALIAS   12
#define MBX_SITE_DD_R        38u
#define MBX_SITE_DD_WALK     39u
#define MBX_SITE_DD_NOISE_A  40u
#define MBX_SITE_DD_NOISE_B  41u

/* ---------------------------------------------------------------- 15. sDMS_PSO (sdms_pso.py) layouts
 * No agent: mbx_reset is __reset (:68-85: random swarm, one evaluation, regroup by a random permutation, lbest per sub-swarm -- NP FEs), every
 * mbx_step (actions = NULL) is one __update (:135-183, NP FEs) plus, in the launch of a generation's tenth update, the generation's epilogue
 * (:220-226: parameter-set push, every tenth generation a regroup with lbest from scratch) and the zeroing of success_num for the next
 * generation.  NP = 99 in 33 sub-swarms of 3 (particle i belongs to sub-swarm i / 3), c1 = c2 = 1.49445, velocity cap 0.1 (ub - lb).
 * cfg.np must be 99, dim <= 40, and max_fes inside the range described at mbx_batch_create's check.  state [1] = fes / maxFEs.
 * state block: X[NP*D] V[NP*D] pbest_pos[NP*D] c_cost[NP] pbest[NP] lbest_pos[33*D] gbest_pos[D] lbest_cost[33] lbest_index[33] success_num[33]
 *   success_last[33] iwt[33] iwt_z[33] parameter_set[8] scalars[16] cost_curve[nlog+1].
 *   success_last:  success_num as the last parameter-set push saw it (success_num itself is zero again after that launch).
 *   iwt / iwt_z:   the inertia weights of the last local-phase update, and the standard normals behind them when they were drawn from
 *                  normal(median(parameter_set), 0.1) (diagnostic: the Philox route makes them with the device's log / cos, which the host does
 *                  not reproduce to the bit; a tape rebuilt from a Philox step takes them from here).
 *   parameter_set: oldest entry first, scalars[MBX_SC_SDMS_NPAR] entries in use (a FIFO of 8).
 *   scalars beyond the common ones (MBX_SC_GEN counts the updates; it is the Philox generation word): the position inside the learning period
 *   (0..9, the number of updates of the running generation already made), the mode (0 local phase, 1 global phase), the inertia weight w of the
 *   global phase, the parameter-set count, how the last update drew iwt (0 uniform, 1 normal, 2 global phase: not drawn), the reference's `gen`.
 * tape per reset: pos_u[NP*D] | vel_u[NP*D] | noise[3*NP] | perm[NP]
 * tape per step:  rand1[NP] | rand2[NP] | iwt_u[33] | iwt_z[33] | noise[3*NP] | perm[NP]
 *   iwt_u is read when __get_iwt draws uniforms, iwt_z (STANDARD normals; the kernel forms median + 0.1 z) when it draws normals, neither in the
 *   global phase; perm (torch.randperm values as doubles, clamped to [0, NP)) in the step that ends a generation whose number is a multiple of 10.
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the step:
 *   MBX_SITE_ELEM_R(e)        reset: u53(w0,w1) = pos_u, u53(w2,w3) = vel_u
 *   MBX_SITE_SD_PART(i)       u53(w0,w1) = rand1, u53(w2,w3) = rand2
 *   MBX_SITE_SD_IWT_U(s)      u53(w0,w1) = iwt_u            MBX_SITE_SD_IWT_Z(s)  Box-Muller of u53(w0,w1), u53(w2,w3): the cosine half = iwt_z
 *   MBX_SITE_SD_PERM(i)       w0 = the key of row i; perm[i] = the rank of key i among the NP keys (equal keys: the lower index first)
 *   MBX_SITE_SD_NOISE_A/B(i)  evaluation of row i (reset and step)                                                                              */
#define MBX_SDMS_NP   99
#define MBX_SDMS_M    3
#define MBX_SDMS_NS   33
#define MBX_SDMS_LP   10
#define MBX_SDMS_LA   8
#define MBX_SDMS_R    10
#define MBX_SDMS_L    100
#define MBX_SDMS_DIM_MAX 40
#define MBX_SDMS_TAPE_POS(NP, D)         ((int64_t)0)
#define MBX_SDMS_TAPE_VEL(NP, D)         ((int64_t)(NP) * (D))
#define MBX_SDMS_TAPE_NOISE_INIT(NP, D)  (2 * (int64_t)(NP) * (D))
#define MBX_SDMS_TAPE_PERM_INIT(NP, D)   (2 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_SDMS_TAPE_RAND1(NP, D)       ((int64_t)0)
#define MBX_SDMS_TAPE_RAND2(NP, D)       ((int64_t)(NP))
#define MBX_SDMS_TAPE_IWT_U(NP, D)       (2 * (int64_t)(NP))
#define MBX_SDMS_TAPE_IWT_Z(NP, D)       (2 * (int64_t)(NP) + MBX_SDMS_NS)
#define MBX_SDMS_TAPE_NOISE(NP, D)       (2 * (int64_t)(NP) + 2 * MBX_SDMS_NS)
#define MBX_SDMS_TAPE_PERM(NP, D)        (5 * (int64_t)(NP) + 2 * MBX_SDMS_NS)
#define MBX_SDMS_TAPE_STRIDE(NP, D)      (2 * (int64_t)(NP) * (D) + 4 * (int64_t)(NP))
#define MBX_SDMS_ST_X(NP, D)             ((int64_t)0)
#define MBX_SDMS_ST_V(NP, D)             ((int64_t)(NP) * (D))
#define MBX_SDMS_ST_PBPOS(NP, D)         (2 * (int64_t)(NP) * (D))
#define MBX_SDMS_ST_CCOST(NP, D)         (3 * (int64_t)(NP) * (D))
#define MBX_SDMS_ST_PBEST(NP, D)         (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_SDMS_ST_LBPOS(NP, D)         (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_SDMS_ST_GBPOS(NP, D)         (MBX_SDMS_ST_LBPOS(NP, D) + (int64_t)MBX_SDMS_NS * (D))
#define MBX_SDMS_ST_LBCOST(NP, D)        (MBX_SDMS_ST_GBPOS(NP, D) + (D))
#define MBX_SDMS_ST_LBIDX(NP, D)         (MBX_SDMS_ST_LBCOST(NP, D) + MBX_SDMS_NS)
#define MBX_SDMS_ST_SUCC(NP, D)          (MBX_SDMS_ST_LBIDX(NP, D) + MBX_SDMS_NS)
#define MBX_SDMS_ST_SUCC_LAST(NP, D)     (MBX_SDMS_ST_SUCC(NP, D) + MBX_SDMS_NS)
#define MBX_SDMS_ST_IWT(NP, D)           (MBX_SDMS_ST_SUCC_LAST(NP, D) + MBX_SDMS_NS)
#define MBX_SDMS_ST_IWT_Z(NP, D)         (MBX_SDMS_ST_IWT(NP, D) + MBX_SDMS_NS)
#define MBX_SDMS_ST_PSET(NP, D)          (MBX_SDMS_ST_IWT_Z(NP, D) + MBX_SDMS_NS)
#define MBX_SDMS_ST_SCALARS(NP, D)       (MBX_SDMS_ST_PSET(NP, D) + MBX_SDMS_LA)
#define MBX_SDMS_STATE_DOUBLES(NP, D, NLOG) (MBX_SDMS_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_SDMS_STEP     10
#define MBX_SC_SDMS_MODE     11
#define MBX_SC_SDMS_W        12
#define MBX_SC_SDMS_NPAR     13
#define MBX_SC_SDMS_IWTMODE  14
#define MBX_SC_SDMS_GEN      15
#define MBX_SITE_SD_PART     42u
#define MBX_SITE_SD_IWT_U    43u
#define MBX_SITE_SD_IWT_Z    44u
#define MBX_SITE_SD_PERM     45u
#define MBX_SITE_SD_NOISE_A  46u
#define MBX_SITE_SD_NOISE_B  47u

/* ---------------------------------------------------------------- 16. NRLPSO (nrlpso_optimizer.py) layouts
 * One env step = ONE particle of the round-robin `pointer` (reset to 0 by init_population, :31).  k = 5 neighbours, v_max = 0.1 (ub - lb),
 * w from the logistic map r_w once per sweep (:88-93, at pointer == 0, with the fes of that moment).  state [1] = the action the next particle took on
 * its previous turn (:278-296; the reset draws randint(0, 4, NP), :58); action [1] int32 in 0..3 (any other value leaves the velocity as it is, :145-191);
 * reward in {2, 1, 0, -2} from (f_new < f_old, ef_new > ef_old) (:95-108).  A step bills 1 FE, or 3 when pbest_stag_count[pointer] >= 2 fires
 * neb_mutation (:271-272), so fes may pass maxFEs by up to 2 and the curve still appends at most once per step (:282-284).
 * The reference's own behaviour, kept:
 *   gbest_pos is a numpy VIEW of population row MBX_SC_NRLPSO_G0 while MBX_SC_NRLPSO_ALIAS is 1: after init_population (:47) and after :276, and it
 *     follows that row when the row moves or a mutation overwrites it (:220, :238); it becomes an array of its own (gbest_pos[D], alias 0) only when
 *     neb_mutation improves gbest (:233).
 *   pbest_cost is not written when a particle improves on it (:265-267 write the position only); only neb_mutation writes it (:216).
 *   pbest_stag_count is not reset by a mutation (:271): once it reaches 2 every later turn of that particle mutates until the particle improves.
 *   pbest_neb / gbest_neb are COPIES taken at pointer == 0 (:75, :84) and go stale within the sweep, while their index lists overwrite LIVE rows
 *     (:219-221, :237-239): the block keeps the sweep-start population `snap` and the index lists, not the NP x k x D rows.
 *   action 3 draws its two random indices and then two rand(D) vectors; the scalars r1, r2 are drawn first all the same and ignored (:138-139, :184-191).
 *   neighbours are chosen by (distance, index); the diagonal of the pbest-to-particle matrix is +inf (:68); a NaN cs or ef compares false.
 * state block: pop[NP*D] vel[NP*D] pbest_pos[NP*D] snap[NP*D] cost[NP] pbest_cost[NP] stag[NP] sstate[NP] pbest_neb_index[NP*5] gbest_neb_index[8]
 *   gbest_pos[D] diag[8] scalars[16] cost_curve[nlog+1].
 *   diag (of the last step): cs | ef_old | ef_new | mutated (0 / 1) | f_new | cost of the pbest mutation | cost of the gbest mutation | action
 * tape per reset: pos_u[NP*D] | noise_init[3*NP] | sstate[NP] | r_w
 * tape per step:  r1 | r2 | idx_b | idx_a | noise[9] | choice_u | r1v[D] | r2v[D] | mut_u1[D] | mut_u2[D]
 *   idx_b / idx_a: the randint(0, k) of get_p_b / get_p_a as doubles (read only where the action and the sign of cs call them); noise: [3][3] rows
 *   (a | b | c) x (the move's evaluation, the pbest mutation's, the gbest mutation's); choice_u: the uniform of the agent's np.random.choice (fused
 *   policy only); r1v / r2v: action 3; mut_u1 / mut_u2: neb_mutation's rand(D) (:212, :230).
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the step:
 *   reset: MBX_SITE_LDE_ELEM(e): u53(w0,w1) = pos_u; noise MBX_SITE_NOISE1_A/B(i); MBX_SITE_NR_INIT(i): mulhi(w0, 4) = sstate[i]; index NP: u53(w0,w1) = r_w
 *   MBX_SITE_NR_PART(0)    u53(w0,w1) = r1, u53(w2,w3) = r2;  index 1: mulhi(w0, 5) = idx_b, mulhi(w1, 5) = idx_a
 *   MBX_SITE_NR_ELEM(d)    u53(w0,w1) = r1v[d], u53(w2,w3) = r2v[d]
 *   MBX_SITE_NR_MUT(d)     u53(w0,w1) = mut_u1[d], u53(w2,w3) = mut_u2[d]
 *   MBX_SITE_NR_NOISE_A/B(j)  evaluation j of the step: 0 the move, 1 the pbest mutation, 2 the gbest mutation
 *   MBX_SITE_POLICY(0)     u53(w0,w1) = choice_u                                                                                              */
#define MBX_NRLPSO_NP_MIN  8
#define MBX_NRLPSO_NP_MAX  128
#define MBX_NRLPSO_DIM_MAX 40
#define MBX_NRLPSO_K       5
#define MBX_NRLPSO_TAPE_POS(NP, D)        ((int64_t)0)
#define MBX_NRLPSO_TAPE_NOISE_INIT(NP, D) ((int64_t)(NP) * (D))
#define MBX_NRLPSO_TAPE_SSTATE(NP, D)     ((int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_NRLPSO_TAPE_RW(NP, D)         ((int64_t)(NP) * (D) + 4 * (int64_t)(NP))
#define MBX_NRLPSO_TAPE_RAND(NP, D)       ((int64_t)0)
#define MBX_NRLPSO_TAPE_IDX(NP, D)        ((int64_t)2)
#define MBX_NRLPSO_TAPE_NOISE(NP, D)      ((int64_t)4)
#define MBX_NRLPSO_TAPE_CHOICE(NP, D)     ((int64_t)13)
#define MBX_NRLPSO_TAPE_R1V(NP, D)        ((int64_t)14)
#define MBX_NRLPSO_TAPE_R2V(NP, D)        ((int64_t)14 + (D))
#define MBX_NRLPSO_TAPE_MUT1(NP, D)       ((int64_t)14 + 2 * (D))
#define MBX_NRLPSO_TAPE_MUT2(NP, D)       ((int64_t)14 + 3 * (D))
#define MBX_NRLPSO_TAPE_STRIDE(NP, D)     ((int64_t)(NP) * (D) + 4 * (int64_t)(NP) + 16)     /* >= 14 + 4 D for np >= 8 */
#define MBX_NRLPSO_ST_POP(NP, D)          ((int64_t)0)
#define MBX_NRLPSO_ST_VEL(NP, D)          ((int64_t)(NP) * (D))
#define MBX_NRLPSO_ST_PBPOS(NP, D)        (2 * (int64_t)(NP) * (D))
#define MBX_NRLPSO_ST_SNAP(NP, D)         (3 * (int64_t)(NP) * (D))
#define MBX_NRLPSO_ST_COST(NP, D)         (4 * (int64_t)(NP) * (D))
#define MBX_NRLPSO_ST_PBCOST(NP, D)       (4 * (int64_t)(NP) * (D) + (NP))
#define MBX_NRLPSO_ST_STAG(NP, D)         (4 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_NRLPSO_ST_SSTATE(NP, D)       (4 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_NRLPSO_ST_PNIDX(NP, D)        (4 * (int64_t)(NP) * (D) + 4 * (int64_t)(NP))
#define MBX_NRLPSO_ST_GNIDX(NP, D)        (MBX_NRLPSO_ST_PNIDX(NP, D) + (int64_t)MBX_NRLPSO_K * (NP))
#define MBX_NRLPSO_ST_GBPOS(NP, D)        (MBX_NRLPSO_ST_GNIDX(NP, D) + 8)
#define MBX_NRLPSO_ST_DIAG(NP, D)         (MBX_NRLPSO_ST_GBPOS(NP, D) + (D))
#define MBX_NRLPSO_DIAG_SLOTS 8
#define MBX_NRLPSO_ST_SCALARS(NP, D)      (MBX_NRLPSO_ST_DIAG(NP, D) + MBX_NRLPSO_DIAG_SLOTS)
#define MBX_NRLPSO_STATE_DOUBLES(NP, D, NLOG) (MBX_NRLPSO_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_NRLPSO_DIAG_CS      0
#define MBX_NRLPSO_DIAG_EF_OLD  1
#define MBX_NRLPSO_DIAG_EF_NEW  2
#define MBX_NRLPSO_DIAG_MUTATED 3
#define MBX_NRLPSO_DIAG_FNEW    4
#define MBX_NRLPSO_DIAG_PMCOST  5
#define MBX_NRLPSO_DIAG_GMCOST  6
#define MBX_NRLPSO_DIAG_ACTION  7
#define MBX_SC_NRLPSO_POINTER 10
#define MBX_SC_NRLPSO_G0      11
#define MBX_SC_NRLPSO_ALIAS   12
#define MBX_SC_NRLPSO_RW      13
#define MBX_SC_NRLPSO_W       14
#define MBX_SITE_NR_PART     48u
#define MBX_SITE_NR_ELEM     49u
#define MBX_SITE_NR_MUT      50u
#define MBX_SITE_NR_NOISE_A  51u
#define MBX_SITE_NR_NOISE_B  52u
#define MBX_SITE_NR_INIT     53u

/* ---------------------------------------------------------------- 17. SAHLPSO (sahlpso.py) layouts
 * No agent: mbx_reset is run_episode :22-47 (V and X draws, 40 evaluations, the static ranking, the 8 exploration particles -- 40 FEs), every
 * mbx_step (actions = NULL) one pass of `for i in remain_index` (:50-124: one move and one FE per live particle, strictly in order, each move
 * seeing the one before it) plus the end-of-generation block (:126-155: every fifth generation the selection probabilities, then the linear
 * population reduction 40 -> 4).  An episode may end in the middle of a pass (:114-124): the later particles stay untouched and fes is exact.
 * cfg.np must be 40, 2 <= dim <= 40, max_fes > 40.  state [1] = fes / maxFEs.  Bounds are the literals -5 / 5, v_max 1 (:10).  Kept behaviour:
 * the header of mbx_sahlpso.hpp.
 * state block: X[40*D] V[40*D] pbest_pos[40*D] f_X[40] pbest_cost0[40] w[40] rank[40] selected[8] P_cr[8] nf_cr[8] ns_cr[8] P_ls[16] nf_ls[16]
 *   ns_ls[16] move_i[40] move_cr[40] move_ls[40] move_succ[40] move_cauchy[40] scalars[16] cost_curve[nlog+1].
 *   pbest_cost0: pBest_cost, which the reference never writes after :31.   rank: np.argsort(pBest_cost) -- rank[k] = the particle with the
 *   k-th smallest initial cost (equal costs: the lower index first); remain_index is 0..39 while NP = 40 and rank[:NP] afterwards, best_p_index
 *   is rank[:max(1, int(0.2 NP))].   selected: selected_indiv_index.   P_cr / nf_cr / ns_cr: 5 entries in use (H_cr stays 5), P_ls / nf_ls / ns_ls: 15.
 *   move_*: one entry per slot of remain_index in the last pass, the first scalars[MBX_SC_SAHL_MOVES] of them valid: the particle, cr_index,
 *   ls_index, the success flag and the standard-cauchy value of a failed move (the Philox route makes it with the device's tan, which the host
 *   does not reproduce to the bit: a tape rebuilt from a Philox step takes it from here).
 *   scalars beyond the common ones (MBX_SC_GEN counts the passes and is the Philox generation word; G = MBX_SC_GEN + 1): the live NP, the row g
 *   of X that gBest views (MBX_SC_GBEST is gBest_cost, which goes stale when row g moves without improving), the moves of the last pass.
 * tape per reset: vel_u[40*D] | pos_u[40*D] | noise[3*40] | selected[8]           (draw order :23, :24, the evaluation, :47)
 * tape per step:  40 records of 10 + 3 D doubles, record k for slot k of remain_index:
 *   u_cr | u_ls | m | n | pick | rnd2 | cauchy | noise a, b, c | cross_u[D] | rnd1[D] | vel_u[D]
 *   u_cr / u_ls: the uniforms of the two np.random.choice(range(H), p=P) (:54, :56; read unless G % 5 == 0 and G != 1); m, n: the two PARTICLES of
 *   np.random.choice(remain_index, 2) (:60, exploration particles), pick: the particle of np.random.choice(best_p_index) (:69, the others), as
 *   doubles, clamped to [0, 40); rnd2 and cauchy (:102-106, the standard_cauchy value itself) are read after a failed move; rnd1 (:76) by the
 *   particles that are not exploration particles.
 * Philox, counter (index, site, gen, episode); reset gen = 0, step gen = number of the pass; k = slot of remain_index:
 *   reset: MBX_SITE_ELEM_R(e): u53(w0,w1) = pos_u, u53(w2,w3) = vel_u;  MBX_SITE_SH_PERM(i): w0 = the key of particle i, selected[r] = the particle
 *          whose key has rank r < 8 among the 40 (equal keys: the lower index first);  noise MBX_SITE_SH_NOISE_A/B(i)
 *   MBX_SITE_SH_CHOICE(k)    u53(w0,w1) = u_cr, u53(w2,w3) = u_ls
 *   MBX_SITE_SH_PICK(k)      remain_index[mulhi(w0, NP)] = m, remain_index[mulhi(w1, NP)] = n, rank[mulhi(w2, len(best_p_index))] = pick
 *   MBX_SITE_SH_ELEM(64 k + d)  u53(w0,w1) = cross_u[d], u53(w2,w3) = rnd1[d]        MBX_SITE_SH_VEL(64 k + d)  u53(w0,w1) = vel_u[d]
 *   MBX_SITE_SH_FAIL(k)      u53(w0,w1) = rnd2, tan(pi (u53(w2,w3) - 0.5)) = cauchy (as MBX_SITE_MD_CAUCHY)
 *   MBX_SITE_SH_NOISE_A/B(k) the evaluation of slot k                                                                                           */
#define MBX_SAHL_NP      40
#define MBX_SAHL_NP_MIN  4
#define MBX_SAHL_DIM_MAX 40
#define MBX_SAHL_NSEL    8
#define MBX_SAHL_HCR     5
#define MBX_SAHL_HLS     15
#define MBX_SAHL_LP      5
#define MBX_SAHL_REC(D)                  (10 + 3 * (int64_t)(D))
#define MBX_SAHL_REC_UCR     0
#define MBX_SAHL_REC_ULS     1
#define MBX_SAHL_REC_M       2
#define MBX_SAHL_REC_N       3
#define MBX_SAHL_REC_PICK    4
#define MBX_SAHL_REC_RND2    5
#define MBX_SAHL_REC_CAUCHY  6
#define MBX_SAHL_REC_NOISE   7
#define MBX_SAHL_REC_CROSS(D)            ((int64_t)10)
#define MBX_SAHL_REC_RND1(D)             (10 + (int64_t)(D))
#define MBX_SAHL_REC_VEL(D)              (10 + 2 * (int64_t)(D))
#define MBX_SAHL_TAPE_VEL(NP, D)         ((int64_t)0)
#define MBX_SAHL_TAPE_POS(NP, D)         ((int64_t)(NP) * (D))
#define MBX_SAHL_TAPE_NOISE_INIT(NP, D)  (2 * (int64_t)(NP) * (D))
#define MBX_SAHL_TAPE_SEL(NP, D)         (2 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_SAHL_TAPE_STRIDE(NP, D)      ((int64_t)(NP) * MBX_SAHL_REC(D))        /* >= 2 NP D + 3 NP + 8 for NP = 40 */
#define MBX_SAHL_ST_X(NP, D)             ((int64_t)0)
#define MBX_SAHL_ST_V(NP, D)             ((int64_t)(NP) * (D))
#define MBX_SAHL_ST_PBPOS(NP, D)         (2 * (int64_t)(NP) * (D))
#define MBX_SAHL_ST_FX(NP, D)            (3 * (int64_t)(NP) * (D))
#define MBX_SAHL_ST_PBCOST0(NP, D)       (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_SAHL_ST_W(NP, D)             (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_SAHL_ST_RANK(NP, D)          (3 * (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_SAHL_ST_SEL(NP, D)           (3 * (int64_t)(NP) * (D) + 4 * (int64_t)(NP))
#define MBX_SAHL_ST_PCR(NP, D)           (MBX_SAHL_ST_SEL(NP, D) + 8)
#define MBX_SAHL_ST_NFCR(NP, D)          (MBX_SAHL_ST_SEL(NP, D) + 16)
#define MBX_SAHL_ST_NSCR(NP, D)          (MBX_SAHL_ST_SEL(NP, D) + 24)
#define MBX_SAHL_ST_PLS(NP, D)           (MBX_SAHL_ST_SEL(NP, D) + 32)
#define MBX_SAHL_ST_NFLS(NP, D)          (MBX_SAHL_ST_SEL(NP, D) + 48)
#define MBX_SAHL_ST_NSLS(NP, D)          (MBX_SAHL_ST_SEL(NP, D) + 64)
#define MBX_SAHL_ST_MOVE_I(NP, D)        (MBX_SAHL_ST_SEL(NP, D) + 80)
#define MBX_SAHL_ST_MOVE_CR(NP, D)       (MBX_SAHL_ST_MOVE_I(NP, D) + (NP))
#define MBX_SAHL_ST_MOVE_LS(NP, D)       (MBX_SAHL_ST_MOVE_I(NP, D) + 2 * (int64_t)(NP))
#define MBX_SAHL_ST_MOVE_SUCC(NP, D)     (MBX_SAHL_ST_MOVE_I(NP, D) + 3 * (int64_t)(NP))
#define MBX_SAHL_ST_MOVE_CAUCHY(NP, D)   (MBX_SAHL_ST_MOVE_I(NP, D) + 4 * (int64_t)(NP))
#define MBX_SAHL_ST_SCALARS(NP, D)       (MBX_SAHL_ST_MOVE_I(NP, D) + 5 * (int64_t)(NP))
#define MBX_SAHL_STATE_DOUBLES(NP, D, NLOG) (MBX_SAHL_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_SAHL_NP       10
#define MBX_SC_SAHL_GROW     11
#define MBX_SC_SAHL_MOVES    12
#define MBX_SITE_SH_CHOICE   54u
#define MBX_SITE_SH_PICK     55u
#define MBX_SITE_SH_ELEM     56u
#define MBX_SITE_SH_VEL      57u
#define MBX_SITE_SH_FAIL     58u
#define MBX_SITE_SH_NOISE_A  59u
#define MBX_SITE_SH_NOISE_B  60u
#define MBX_SITE_SH_PERM     61u

/* ---------------------------------------------------------------- 18. LES (les_optimizer.py) layouts
 * A learned evolution strategy: a 68-parameter attention module turns the 16 costs of a generation into recombination weights W, a
 * 178-parameter MLP turns the evolution paths and a timestamp embedding into per-coordinate learning rates, and a diagonal Gaussian (mu, sigma)
 * is sampled 16 times per generation.  mbx_reset is init_population (:63-84: D uniforms, 16 D normals, 16 FEs); one generation is one turn of
 * update()'s loop (:128-178, 16 FEs).  mbx_les_rollout runs n_gens of them in one launch with everything below in LDS; mbx_step (actions = NULL)
 * is one generation.  The 246 float32 parameters are PER INSTANCE: mbx_les_set_params stores n_sets vectors and one set index per instance.
 * cfg.np must be 16, 2 <= dim <= 40, max_fes > 16.  state [1] = gbest.  Costs are problem.eval(x) as the reference takes them: noise included,
 * the optimum NOT subtracted (:71, :147).  Kept behaviour and the float32 summation orders: the header of mbx_les.hpp.
 * state block: parents[16*D] parents_cost[16] mu[D] sigma[D] Pc[3*D] Ps[3*D] normals[16*D] W[16] alpha[2*D] scalars[16] cost_curve[MBX_LES_CURVE_CAP].
 *   normals: the standard normals z of the LAST sampling (parents = clip(mu + sigma z)), so that a Philox run can be fed back as a tape;
 *   W: the attention weights of the last generation, alpha[2 d + k]: its learning rates (k = 0 mu, 1 sigma) -- float32 values held in doubles.
 *   scalars beyond the common ones (MBX_SC_GEN is evolution_info['generation_counter'] and, plus one, the Philox generation word): init_y of the
 *   budget route (gbest after the first generation after the reset) and init_y of the running skip_step call (gbest after its first generation).
 * tape per reset:      mu_u[D] | z[16*D] | noise[3*16]            (draw order :68, :70, the evaluation)
 * tape per generation: z[16*D] | noise[3*16]                      (:145, the evaluation); np.random.normal(mu, sigma, (16, D)) is mu + sigma * gauss
 *   element by element in C order.  A tape holds one generation: with a tape n_gens must be 1.
 * Philox, counter (index, site, gen, episode); reset gen = 0, a generation gen = generation_counter + 1 (the counter BEFORE the generation):
 *   MBX_SITE_LES_MU(d)       u53(w0,w1) = mu_u[d]                                  (reset only)
 *   MBX_SITE_LES_NORMAL(p)   box_muller(u53(w0,w1), u53(w2,w3)) = z[2 p], z[2 p + 1]   (16 D is even)
 *   MBX_SITE_LES_NOISE_A/B(i) the evaluation of row i                                                                                         */
#define MBX_LES_NP       16
#define MBX_LES_DIM_MAX  40
#define MBX_LES_NPARAM   246     /* attn[0:68] = Wq.weight (8x3), Wq.bias, Wk.weight, Wk.bias, Wv.weight (1x3), Wv.bias; mlp[68:246] = ln1.weight (8x19), ln1.bias, ln2.weight (2x8), ln2.bias */
#define MBX_LES_NATTN    68
#define MBX_LES_NTS      13      /* timestamps 1, 3, 10, 30, 50, 100, 250, 500, 750, 1000, 1250, 1500, 2000 (:51) */
#define MBX_LES_TS_MARGIN 64     /* the timestamp table holds generation counters 0 .. max_fes / 16 + MBX_LES_TS_MARGIN; past it (skip_step calls far beyond the budget) the kernel takes the device's tanh */
#define MBX_LES_TAPE_MU(NP, D)           ((int64_t)0)
#define MBX_LES_TAPE_Z0(NP, D)           ((int64_t)(D))
#define MBX_LES_TAPE_NOISE_INIT(NP, D)   ((int64_t)(D) + (int64_t)(NP) * (D))
#define MBX_LES_TAPE_Z(NP, D)            ((int64_t)0)
#define MBX_LES_TAPE_NOISE(NP, D)        ((int64_t)(NP) * (D))
#define MBX_LES_TAPE_STRIDE(NP, D)       ((int64_t)(D) + (int64_t)(NP) * (D) + 3 * (int64_t)(NP))
#define MBX_LES_ST_PARENTS(NP, D)        ((int64_t)0)
#define MBX_LES_ST_COST(NP, D)           ((int64_t)(NP) * (D))
#define MBX_LES_ST_MU(NP, D)             ((int64_t)(NP) * (D) + (NP))
#define MBX_LES_ST_SIGMA(NP, D)          (MBX_LES_ST_MU(NP, D) + (D))
#define MBX_LES_ST_PC(NP, D)             (MBX_LES_ST_MU(NP, D) + 2 * (int64_t)(D))
#define MBX_LES_ST_PS(NP, D)             (MBX_LES_ST_MU(NP, D) + 5 * (int64_t)(D))
#define MBX_LES_ST_Z(NP, D)              (MBX_LES_ST_MU(NP, D) + 8 * (int64_t)(D))
#define MBX_LES_ST_W(NP, D)              (MBX_LES_ST_Z(NP, D) + (int64_t)(NP) * (D))
#define MBX_LES_ST_ALPHA(NP, D)          (MBX_LES_ST_W(NP, D) + (NP))
#define MBX_LES_ST_SCALARS(NP, D)        (MBX_LES_ST_ALPHA(NP, D) + 2 * (int64_t)(D))
/* The reference's cost list can grow past n_logpoint + 1: the log point (:170-172) appends once per generation whenever FEs has reached it, unguarded, and
 * only the closing entry (:174-178) looks at the length (maxFEs = 976, log_interval = 976 // 50 = 19: 52 entries).  The curve of an LES instance therefore has
 * MBX_LES_CURVE_CAP slots: what an episode that runs to its budget can append (one entry per generation or per log interval, whichever is fewer, plus the first and
 * the closing one), never fewer than n_logpoint + 1.  mbx_results / mbx_read_public report the first n_logpoint + 1 entries and the true length. */
#define MBX_LES_GENS(MAXFES)             (((int64_t)(MAXFES) - 1) / MBX_LES_NP)                    /* generations until FEs >= maxFEs */
#define MBX_LES_FIRES(MAXFES, LOGINT)    (((MBX_LES_GENS(MAXFES) + 1) * MBX_LES_NP / (LOGINT)) < MBX_LES_GENS(MAXFES) ? ((MBX_LES_GENS(MAXFES) + 1) * MBX_LES_NP / (LOGINT)) : MBX_LES_GENS(MAXFES))
#define MBX_LES_CURVE_CAP(MAXFES, LOGINT, NLOG) (MBX_LES_FIRES(MAXFES, LOGINT) + 2 > (int64_t)(NLOG) + 1 ? MBX_LES_FIRES(MAXFES, LOGINT) + 2 : (int64_t)(NLOG) + 1)
#define MBX_LES_STATE_DOUBLES(NP, D, CAP) (MBX_LES_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(CAP))
#define MBX_SC_LES_INIT_Y      10
#define MBX_SC_LES_CALL_INIT_Y 11
#define MBX_SITE_LES_MU      62u
#define MBX_SITE_LES_NORMAL  63u
#define MBX_SITE_LES_NOISE_A 64u
#define MBX_SITE_LES_NOISE_B 65u

/* ---------------------------------------------------------------- 19. RL-HPSDE (rl_hpsde_optimizer.py) layouts
 * SHADE-style DE with a success-history memory MF / MCr of H = int(0.5 D) entries, linear population size reduction from N0 = 18 D rows towards 4,
 * and a tabular agent whose action picks the mutation (action & 1: cur_to_rand_1 / cur_to_best_1) and the law of F (action >> 1: Cauchy / Levy).
 * After the reset and after EVERY update a progressive random walk of 201 points is drawn, evaluated and billed, and two landscape bits make the
 * state = DFDC + 2 DRIE in 0..3.  mbx_reset is init_population (:123-131), mbx_step one update (:231-287) with the caller's int32 action,
 * mbx_rlhpsde_rollout (include/mbx_rlhpsde.h) n_steps updates in one launch with the 4 x 4 Q-table.  cfg.np must be 18 dim, 2 <= dim <= 40,
 * max_fes > np + 201.  state [1] = the landscape state, action [1] int32.  Rules and the quirks kept: the header of mbx_rlhpsde.hpp.
 * state block: pop[2][N0*D] (two buffers, MBX_SC_HP_LIVE names the live one; rows sorted by (cost, row)) cost[N0] MF[H] MCr[H] u[N0*D] (trial rows)
 *   ncost[N0] F[N0] Cr[N0] r[3*N0] (the indices of the last mutation, r[3 i + c]) z[N0] x[N0] (the standard normal behind Cr and the Cauchy / Levy
 *   variate behind F of the last update, so that a Philox run can be fed back as a tape) walk[201*D] wcost[201] feat[MBX_RLHPSDE_FEAT_SLOTS]
 *   scalars[16] cost_curve[n_logpoint + 1].  feat: the correlation r, the entropy, its level, the improved rows of the last update, then the
 *   transition counts count[level][class] of the nine levels (classes in the reference's order: -1>0, -1>1, 0>-1, 0>1, 1>-1, 1>0).
 * The tape has one walk section in front, shared by reset and step, then the reset's or the step's own part:
 *   walk:  zone_u[D] | off_u[D] | step_u[200*D] | rD | choice_u | wnoise[3*201]      (draw order :152, :155, :157, :163; choice_u: the agent's uniform,
 *          read by mbx_rlhpsde_rollout only)
 *   reset: pos_u[N0*D] | noise[3*N0]
 *   step:  mem[N0] | z[N0] | x[N0] | r[3*N0] | jrand[N0] | noise[3*N0] | cross_u[N0*D]    (rows past the live NP are not read)
 *          z: the standard normal behind Cr (Cr = clip(MCr[mem] + 0.1 z)); x: the standard Cauchy or Levy variate (F = 0.1 x + MF[mem]);
 *          r: the RESOLVED indices of generate_random_int (mutate.py:12-33), r[3 i + c]; column 2 is not read by cur_to_best_1.
 * A tape holds one update: with a tape n_steps must be 1.
 * Philox, counter (index, site, gen, episode); reset gen = 0, update gen = number of the update:
 *   MBX_SITE_HP_PAR(i)        mulhi(w0, H) = mem, mulhi(w1, D) = jrand
 *   MBX_SITE_HP_NORM(i)       box_muller(u53(w0,w1), u53(w2,w3)): the cosine half = z, the sine half s gives the Levy variate x = 1 / s^2
 *   MBX_SITE_HP_CAUCHY(i)     tan(pi (u53(w0,w1) - 0.5)) = the Cauchy variate x
 *   MBX_SITE_HP_IDX(i*32+a)   attempt a = 0..25 of the bounded redraw: mulhi(w0, NP) = r0, mulhi(w1, NP) = r1, mulhi(w2, NP) = r2, each column with
 *                             its own attempt counter
 *   MBX_SITE_HP_CROSS(i*D+d)  u53(w0,w1) = cross_u;  reset: index e, u53(w0,w1) = pos_u
 *   MBX_SITE_HP_NOISE_A/B(i)  evaluation of trial row i;  reset: MBX_SITE_NOISE1_A/B(i)
 *   MBX_SITE_HP_WALK(e)       e < D: u53(w0,w1) = zone_u[e], u53(w2,w3) = off_u[e];  e = D + k: u53(w0,w1) = step_u[k];  e = 201 D: mulhi(w0, D) = rD
 *   MBX_SITE_HP_WNOISE_A/B(j) evaluation of walk point j
 *   MBX_SITE_POLICY(0)        u53(w0,w1) = choice_u                                                                                             */
#define MBX_RLHPSDE_NP(D)                (18 * (D))
#define MBX_RLHPSDE_DIM_MAX              40
#define MBX_RLHPSDE_MEM(D)                 ((int64_t)((D) / 2))
#define MBX_RLHPSDE_WALK                 201     /* rw_steps + 1 points */
#define MBX_RLHPSDE_NLEVEL               9
#define MBX_RLHPSDE_NCLASS               6
#define MBX_RLHPSDE_FEAT_R               0
#define MBX_RLHPSDE_FEAT_H               1
#define MBX_RLHPSDE_FEAT_LEVEL           2
#define MBX_RLHPSDE_FEAT_NOPT            3
#define MBX_RLHPSDE_FEAT_COUNTS          10
#define MBX_RLHPSDE_FEAT_SLOTS           64
#define MBX_RLHPSDE_TAPE_ZONE(NP, D)     ((int64_t)0)
#define MBX_RLHPSDE_TAPE_OFF(NP, D)      ((int64_t)(D))
#define MBX_RLHPSDE_TAPE_STEPU(NP, D)    (2 * (int64_t)(D))
#define MBX_RLHPSDE_TAPE_RD(NP, D)       (202 * (int64_t)(D))
#define MBX_RLHPSDE_TAPE_CHOICE(NP, D)   (202 * (int64_t)(D) + 1)
#define MBX_RLHPSDE_TAPE_WNOISE(NP, D)   (202 * (int64_t)(D) + 2)
#define MBX_RLHPSDE_TAPE_BASE(NP, D)     (202 * (int64_t)(D) + 2 + 3 * MBX_RLHPSDE_WALK + 1)
#define MBX_RLHPSDE_TAPE_POS(NP, D)      MBX_RLHPSDE_TAPE_BASE(NP, D)
#define MBX_RLHPSDE_TAPE_NOISE_INIT(NP, D) (MBX_RLHPSDE_TAPE_BASE(NP, D) + (int64_t)(NP) * (D))
#define MBX_RLHPSDE_TAPE_MEM(NP, D)      MBX_RLHPSDE_TAPE_BASE(NP, D)
#define MBX_RLHPSDE_TAPE_Z(NP, D)        (MBX_RLHPSDE_TAPE_BASE(NP, D) + (int64_t)(NP))
#define MBX_RLHPSDE_TAPE_X(NP, D)        (MBX_RLHPSDE_TAPE_BASE(NP, D) + 2 * (int64_t)(NP))
#define MBX_RLHPSDE_TAPE_R(NP, D)        (MBX_RLHPSDE_TAPE_BASE(NP, D) + 3 * (int64_t)(NP))
#define MBX_RLHPSDE_TAPE_JRAND(NP, D)    (MBX_RLHPSDE_TAPE_BASE(NP, D) + 6 * (int64_t)(NP))
#define MBX_RLHPSDE_TAPE_NOISE(NP, D)    (MBX_RLHPSDE_TAPE_BASE(NP, D) + 7 * (int64_t)(NP))
#define MBX_RLHPSDE_TAPE_CROSS(NP, D)    (MBX_RLHPSDE_TAPE_BASE(NP, D) + 10 * (int64_t)(NP))
#define MBX_RLHPSDE_TAPE_STRIDE(NP, D)   (MBX_RLHPSDE_TAPE_BASE(NP, D) + 10 * (int64_t)(NP) + (int64_t)(NP) * (D))
#define MBX_RLHPSDE_ST_POP(NP, D)        ((int64_t)0)
#define MBX_RLHPSDE_ST_COST(NP, D)       (2 * (int64_t)(NP) * (D))
#define MBX_RLHPSDE_ST_MF(NP, D)         (MBX_RLHPSDE_ST_COST(NP, D) + (NP))
#define MBX_RLHPSDE_ST_MCR(NP, D)        (MBX_RLHPSDE_ST_MF(NP, D) + MBX_RLHPSDE_MEM(D))
#define MBX_RLHPSDE_ST_U(NP, D)          (MBX_RLHPSDE_ST_MCR(NP, D) + MBX_RLHPSDE_MEM(D))
#define MBX_RLHPSDE_ST_NCOST(NP, D)      (MBX_RLHPSDE_ST_U(NP, D) + (int64_t)(NP) * (D))
#define MBX_RLHPSDE_ST_F(NP, D)          (MBX_RLHPSDE_ST_NCOST(NP, D) + (NP))
#define MBX_RLHPSDE_ST_CR(NP, D)         (MBX_RLHPSDE_ST_F(NP, D) + (NP))
#define MBX_RLHPSDE_ST_R(NP, D)          (MBX_RLHPSDE_ST_CR(NP, D) + (NP))
#define MBX_RLHPSDE_ST_Z(NP, D)          (MBX_RLHPSDE_ST_R(NP, D) + 3 * (int64_t)(NP))
#define MBX_RLHPSDE_ST_X(NP, D)          (MBX_RLHPSDE_ST_Z(NP, D) + (NP))
#define MBX_RLHPSDE_ST_WALK(NP, D)       (MBX_RLHPSDE_ST_X(NP, D) + (NP))
#define MBX_RLHPSDE_ST_WCOST(NP, D)      (MBX_RLHPSDE_ST_WALK(NP, D) + MBX_RLHPSDE_WALK * (int64_t)(D))
#define MBX_RLHPSDE_ST_FEAT(NP, D)       (MBX_RLHPSDE_ST_WCOST(NP, D) + MBX_RLHPSDE_WALK)
#define MBX_RLHPSDE_ST_SCALARS(NP, D)    (MBX_RLHPSDE_ST_FEAT(NP, D) + MBX_RLHPSDE_FEAT_SLOTS)
#define MBX_RLHPSDE_STATE_DOUBLES(NP, D, NLOG) (MBX_RLHPSDE_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_HP_NP       10
#define MBX_SC_HP_K        11
#define MBX_SC_HP_LIVE     12
#define MBX_SC_HP_STATE    13
#define MBX_SC_HP_ACTION   14
#define MBX_SITE_HP_PAR      66u
#define MBX_SITE_HP_NORM     67u
#define MBX_SITE_HP_CAUCHY   68u
#define MBX_SITE_HP_IDX      69u
#define MBX_SITE_HP_CROSS    70u
#define MBX_SITE_HP_NOISE_A  71u
#define MBX_SITE_HP_NOISE_B  72u
#define MBX_SITE_HP_WALK     73u
#define MBX_SITE_HP_WNOISE_A 74u
#define MBX_SITE_HP_WNOISE_B 75u

/* ---------------------------------------------------------------- 20. NL_SHADE_LBC (nl_shade_lbc.py) layouts
 * SHADE-style DE, a classic baseline without an agent: success-history memory MF / MCr of H = 20 D entries, an archive of up to N0 rows, a population that
 * shrinks non-linearly from N0 = 23 D rows to 4, rank-weighted r2, a binomial and an exponential crossover computed side by side.  mbx_reset is
 * __init_population (:149-160), mbx_step (actions = NULL) one __update (:163-273), mbx_nlshade_run (include/mbx_nlshade.h) n updates in one launch.
 * cfg.np must be 23 dim, 2 <= dim <= 40, max_fes > np.  state [1] = fes / max_fes, no action.  Rules and the quirks kept: the header of mbx_nlshade.hpp.
 * The population schedule is a per-batch table built by the host at mbx_batch_create (bp.pci: count G, then N after update 0 .. G, long double power).
 * state block: pop[2][N0*D] (two buffers, MBX_SC_NL_LIVE names the live one; rows sorted by (cost, row)) cost[N0] arc[N0*D] MF[H] MCr[H] u[N0*D] (trial
 *   rows) ncost[N0] F[N0] Cr[N0] (SORTED ascending, Cr[i] is row i's) idx[4*N0] (pbs, r1, r2, archive index of the last mutation, idx[4 i + c]; -1 where
 *   the row did not use it) z[N0] c[N0] u2[N0] (the standard normal behind Cr, the Cauchy variate behind F and the uniform behind r2 of the last update,
 *   so that a Philox run can be fed back as a tape) carry[2] (pb, NA: what __init_population does not reset; carry[0] == 0 marks a new batch, which
 *   starts at pb = 0.4, NA = N0) scalars[16] cost_curve[n_logpoint + 1].
 * tape:  reset: pos_u[N0*D] | noise[3*N0]
 *        step:  mem[N0] | z[N0] | c[N0] | pbs[N0] | r1[N0] | u2[N0] | rvs[N0] | aidx[N0] | jrand[N0] | L[N0] | pick[N0] | noise[3*N0] | arcw[N0] |
 *               crossb_u[N0*D] | crosse_u[N0*D]          (rows past the live NP are not read)
 *          pbs, r1, aidx: the RESOLVED indices (after the bounded redraws); u2: the uniform of the KEPT np.random.choice draw, the kernel builds the
 *          cdf and searches it; pick: rand(NP), > 0.5 takes the exponential crossover; arcw[k]: the archive row the improved row of rank k overwrites.
 * A tape holds one update: with a tape n_updates must be 1.
 * Philox, counter (index, site, gen, episode); reset gen = 0, update gen = number of the update:
 *   MBX_SITE_NL_PAR(i)        mulhi(w0, H) = mem, mulhi(w1, D) = jrand, mulhi(w2, D) = L, w3 / 2^32 = pick
 *   MBX_SITE_NL_NORM(i)       box_muller(u53(w0,w1), u53(w2,w3)): the cosine half = z
 *   MBX_SITE_NL_CAUCHY(i)     tan(pi (u53(w0,w1) - 0.5)) = c, u53(w2,w3) = rvs
 *   MBX_SITE_NL_IDX(i*32+a)   attempt a of the bounded redraws, each index with its own attempt counter: pbs = mulhi(w0, pb_upper) at a = 0 and
 *                             mulhi(w0, NP) at a = 1 (one redraw); r1 = mulhi(w1, NP), a = 0..25; u2 = u53(w2,w3), a = 0..25
 *   MBX_SITE_NL_ARC(i)        mulhi(w0, rows) = arcw[i], mulhi(w1, rows) = aidx of row i
 *   MBX_SITE_NL_CROSS(i*D+d)  u53(w0,w1) = crossb_u, u53(w2,w3) = crosse_u;  reset: index e, u53(w0,w1) = pos_u
 *   MBX_SITE_NL_NOISE_A/B(i)  evaluation of trial row i;  reset: MBX_SITE_NOISE1_A/B(i)                                                        */
#define MBX_NLSHADE_NP(D)                (23 * (D))
#define MBX_NLSHADE_DIM_MAX              40
#define MBX_NLSHADE_H(D)                 (20 * (int64_t)(D))
#define MBX_NLSHADE_TAPE_POS(NP, D)      ((int64_t)0)
#define MBX_NLSHADE_TAPE_NOISE_INIT(NP, D) ((int64_t)(NP) * (D))
#define MBX_NLSHADE_TAPE_MEM(NP, D)      ((int64_t)0)
#define MBX_NLSHADE_TAPE_Z(NP, D)        ((int64_t)(NP))
#define MBX_NLSHADE_TAPE_C(NP, D)        (2 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_PBS(NP, D)      (3 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_R1(NP, D)       (4 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_U2(NP, D)       (5 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_RVS(NP, D)      (6 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_AIDX(NP, D)     (7 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_JRAND(NP, D)    (8 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_L(NP, D)        (9 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_PICK(NP, D)     (10 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_NOISE(NP, D)    (11 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_ARCW(NP, D)     (14 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_CROSSB(NP, D)   (15 * (int64_t)(NP))
#define MBX_NLSHADE_TAPE_CROSSE(NP, D)   (15 * (int64_t)(NP) + (int64_t)(NP) * (D))
#define MBX_NLSHADE_TAPE_STRIDE(NP, D)   (15 * (int64_t)(NP) + 2 * (int64_t)(NP) * (D))
#define MBX_NLSHADE_ST_POP(NP, D)        ((int64_t)0)
#define MBX_NLSHADE_ST_COST(NP, D)       (2 * (int64_t)(NP) * (D))
#define MBX_NLSHADE_ST_ARC(NP, D)        (MBX_NLSHADE_ST_COST(NP, D) + (NP))
#define MBX_NLSHADE_ST_MF(NP, D)         (MBX_NLSHADE_ST_ARC(NP, D) + (int64_t)(NP) * (D))
#define MBX_NLSHADE_ST_MCR(NP, D)        (MBX_NLSHADE_ST_MF(NP, D) + MBX_NLSHADE_H(D))
#define MBX_NLSHADE_ST_U(NP, D)          (MBX_NLSHADE_ST_MCR(NP, D) + MBX_NLSHADE_H(D))
#define MBX_NLSHADE_ST_NCOST(NP, D)      (MBX_NLSHADE_ST_U(NP, D) + (int64_t)(NP) * (D))
#define MBX_NLSHADE_ST_F(NP, D)          (MBX_NLSHADE_ST_NCOST(NP, D) + (NP))
#define MBX_NLSHADE_ST_CR(NP, D)         (MBX_NLSHADE_ST_F(NP, D) + (NP))
#define MBX_NLSHADE_ST_IDX(NP, D)        (MBX_NLSHADE_ST_CR(NP, D) + (NP))
#define MBX_NLSHADE_ST_Z(NP, D)          (MBX_NLSHADE_ST_IDX(NP, D) + 4 * (int64_t)(NP))
#define MBX_NLSHADE_ST_C(NP, D)          (MBX_NLSHADE_ST_Z(NP, D) + (NP))
#define MBX_NLSHADE_ST_U2(NP, D)         (MBX_NLSHADE_ST_C(NP, D) + (NP))
#define MBX_NLSHADE_ST_CARRY(NP, D)      (MBX_NLSHADE_ST_U2(NP, D) + (NP))
#define MBX_NLSHADE_ST_SCALARS(NP, D)    (MBX_NLSHADE_ST_CARRY(NP, D) + 2)
#define MBX_NLSHADE_STATE_DOUBLES(NP, D, NLOG) (MBX_NLSHADE_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)
#define MBX_SC_NL_NP       10
#define MBX_SC_NL_ARC      11
#define MBX_SC_NL_K        12
#define MBX_SC_NL_LIVE     13
#define MBX_SITE_NL_PAR      76u
#define MBX_SITE_NL_NORM     77u
#define MBX_SITE_NL_CAUCHY   78u
#define MBX_SITE_NL_IDX      79u
#define MBX_SITE_NL_ARC      80u
#define MBX_SITE_NL_CROSS    81u
#define MBX_SITE_NL_NOISE_A  82u
#define MBX_SITE_NL_NOISE_B  83u

/* ---------------------------------------------------------------- 21. L2L (l2l_optimizer.py, l2l_agent.py:92-135) layouts
 * MBX_ALGO_L2L (26), np = 1, dim <= 40.  An episode is at most MBX_L2L_T = 100 strictly sequential steps (the reference's literal: max_fes plays no
 * part); a step is one cell of nn.LSTM(input D + 2, hidden 32, proj D) in float64, the box map lb + (ub - lb) * (1 / (1 + exp(-x_raw))) and ONE
 * evaluation y = problem.eval(x) [- optimum], noise included.  mbx_l2l_rollout runs n_steps of them in one launch with everything below in LDS;
 * mbx_step (actions = x_raw [B, D] float64) is the box map, the evaluation and the bookkeeping alone: the host ran the cell.
 * Weights are PER INSTANCE SET (mbx_l2l_set_params), one set = MBX_L2L_NPARAM(D) float64 in torch's order:
 *   weight_ih_l0 [128][D + 2] | weight_hh_l0 [128][D] | bias_ih_l0 [128] | bias_hh_l0 [128] | weight_hr_l0 [D][32];  gate rows i | f | g | o, 32 each.
 * state block: in[D + 2] h[D] c[32] x[D] scalars[16] cost_curve[MBX_L2L_CURVE_CAP].
 *   in:  the cell's next input (x_raw, y, constant); all zeros after mbx_reset -- the constant slot is 0 at step 0 and 1 from step 1 on.
 *   h:   the projected hidden state = the last x_raw;  c: the cell state;  x: the last evaluated position (diagnostic).
 *   scalars: MBX_SC_GBEST = best y so far (strict <), MBX_SC_FES = MBX_SC_GEN = steps executed, MBX_SC_COST_LEN = ceil(steps / 2), MBX_SC_DONE,
 *            MBX_SC_RETURN = sum y / y_0, and the three below.
 *   cost_curve: the reference's cost[::2] -- slot k (0 <= k < 50) = best after step 2 k + 1; readers pad the later slots with the last real entry.
 *   done = (optimum known and early_stop and y <= 1e-8) or steps >= 100; a finished instance stays frozen.
 * Summation order (float64, no contraction: every product is rounded, then added):
 *   s1 = sum_j W_ih[r][j] in[j], j ascending from 0.0;  s2 = sum_j W_hh[r][j] h[j] likewise;  gate_r = ((s1 + b_ih[r]) + s2) + b_hh[r];
 *   sigmoid(v) = 1 / (1 + exp(-v));  c' = sigmoid(f) * c + sigmoid(i) * tanh(g);  x_raw[d] = sum_k W_hr[d][k] (sigmoid(o_k) * tanh(c'_k)), k ascending from 0.0.
 * tape (per step): the evaluator's draws for one row, noise[3] (a | b | c as every other tape's noise rows).
 * Philox: the single-row noise sites MBX_SITE_NOISE0_A/B, index 0, counter word 2 (generation) = the 1-based step.                              */
#define MBX_L2L_DIM_MAX  40
#define MBX_L2L_HID      32
#define MBX_L2L_GATES    128
#define MBX_L2L_T        100
#define MBX_L2L_CURVE    50
#define MBX_L2L_NPARAM(D)            (MBX_L2L_GATES * ((int64_t)(D) + 2) + MBX_L2L_GATES * (int64_t)(D) + 2 * MBX_L2L_GATES + (int64_t)(D) * MBX_L2L_HID)
#define MBX_L2L_W_IH(D)              ((int64_t)0)
#define MBX_L2L_W_HH(D)              (MBX_L2L_GATES * ((int64_t)(D) + 2))
#define MBX_L2L_B_IH(D)              (MBX_L2L_W_HH(D) + MBX_L2L_GATES * (int64_t)(D))
#define MBX_L2L_B_HH(D)              (MBX_L2L_B_IH(D) + MBX_L2L_GATES)
#define MBX_L2L_W_HR(D)              (MBX_L2L_B_HH(D) + MBX_L2L_GATES)
#define MBX_L2L_TAPE_NOISE(NP, D)    ((int64_t)0)
#define MBX_L2L_TAPE_STRIDE(NP, D)   ((int64_t)3)
#define MBX_L2L_ST_IN(NP, D)         ((int64_t)0)
#define MBX_L2L_ST_H(NP, D)          ((int64_t)(D) + 2)
#define MBX_L2L_ST_C(NP, D)          (2 * (int64_t)(D) + 2)
#define MBX_L2L_ST_X(NP, D)          (2 * (int64_t)(D) + 2 + MBX_L2L_HID)
#define MBX_L2L_ST_SCALARS(NP, D)    (3 * (int64_t)(D) + 2 + MBX_L2L_HID)
#define MBX_L2L_CURVE_CAP(NLOG)      ((int64_t)(NLOG) + 1 > MBX_L2L_CURVE ? (int64_t)(NLOG) + 1 : (int64_t)MBX_L2L_CURVE)
#define MBX_L2L_STATE_DOUBLES(NP, D, NLOG) (MBX_L2L_ST_SCALARS(NP, D) + MBX_NSCALAR + MBX_L2L_CURVE_CAP(NLOG))
#define MBX_SC_L2L_YSUM  10   /* sum of y over the executed steps */
#define MBX_SC_L2L_Y0    11   /* y of step 1 */
#define MBX_SC_L2L_Y     12   /* y of the last step */

/* ---------------------------------------------------------------- 22. SYMBOL (symbol_optimizer.py, symbol_related/population.py) layouts
 * MBX_ALGO_SYMBOL (27), np in [4, 128], dim in [2, 40].  An action is an UPDATE RULE, a heap-ordered expression tree of MBX_SYM_SLOTS = 2^6 - 1 slots
 * (children of p at 2p + 1 and 2p + 2, -1 = empty) over the tokens below with a float64 constant per slot, applied for n_substeps (the reference: 5)
 * sub-steps: next = x + f(x, gb, gw, dx, randx.., pb), the periodic wrap lb + floored_mod(next - ub, ub - lb), one evaluation of the NP rows and
 * Population.update.  The tree is evaluated as the reference's parenthesised infix string is: (left op right), -(child), float64, no contraction.
 * tokens: 0 '+', 1 '*' (binary), 2 '-' (unary, left child only), 3 'C-1', 4 'C0' (constants: the value is consts[slot], already scaled by its
 *         power of ten), 5 x, 6 gb, 7 gw, 8 dx (= delta_x), 9 randx, 10 pb.  The k-th randx leaf in post-order (= left to right in the string) gathers whole rows
 *         of the PRE-MOVE x by the k-th index row of the sub-step.  mbx_step takes the program as [B, 126] float64: 63 tokens, then 63 constants.
 * A malformed program (empty or leaf root, unknown token, operator with an empty child or below slot 31, a node under a leaf / an empty slot / on the
 * right of a unary) leaves the instance untouched and sets d_n_bad.
 * state block: x[NP*D] pbest_pos[NP*D] delta_x[NP*D] cost[NP] pbest[NP] gbest_pos[D] gworst_pos[D] cbest_pos[D] feat[10] scalars[16]
 *              cost_curve[n_logpoint+1] idx[MBX_SYM_SUB_MAX][MBX_SYM_RANDX_MAX][NP] as BYTES (the index rows the last action drew, sub-step major).
 *   feat: the nine features of feature_encoding (population.py:175-209) after the last completed action (or the reset); slot 9 is padding.
 *   scalars beyond the common ones (MBX_SC_GEN counts the sub-steps of the episode; plus one it is the Philox generation word): the sub-steps done of
 *   the action in progress, gworst_cost, cbest_cost, cbest_index, stag_count, pre_gbest, init_cost.
 * tape: pos_u[NP*D] (x = -ub + (ub - -ub) u, Population.reset) noise_init[3*NP], then per sub-step s < MBX_SYM_SUB_MAX: idx[32][NP] (as doubles) noise[3*NP].
 * Philox: reset (gen 0): MBX_SITE_ELEM_R(e): u53(w0,w1) = pos_u; noise MBX_SITE_NOISE1_A/B(i).
 *         sub-step: MBX_SITE_SYM_IDX(k*NP + i): mulhi(w0, NP) = index i of randx occurrence k; noise MBX_SITE_NOISE0_A/B(i).
 * Features, in the kernel's order (np_sum = numpy's pairwise block, mbx_npsum.hpp): den = gworst - gbest + 1e-8, maxd = sqrt((ub - lb)^2 D);
 *   f1 = np_sum_i((c_i - gbest) / den) / NP;  f2 = (np_sum_i(np_sum_j |x_i - x_j|) / (NP NP)) / maxd, |.| = sqrt of the squares summed d ascending from 0.;
 *   f3 = std(c) / (std(fit) + 1e-8), std(v) = sqrt(np_sum((v - np_sum(v) / NP)^2) / NP), fit = gworst for i < NP / 2, else gbest;
 *   f4 = (max_fes - fes) / max_fes;  f5 = stag / (max_fes / NP, integers);  f6 / f8 = np_sum_i(sqrt(np_sum_d (x_id - p_d)^2) / maxd) / NP for p = cbest / gbest position;
 *   f7 = np_sum_i((c_i - cbest) / den) / NP;  f9 = gbest < pre_gbest.                                                                                  */
#define MBX_SYM_DIM_MAX    40
#define MBX_SYM_NP_MAX     128
#define MBX_SYM_SLOTS      63
#define MBX_SYM_NTOK       11
#define MBX_SYM_RANDX_MAX  32
#define MBX_SYM_SUB_MAX    8
#define MBX_SYM_SKIP       5     /* sub-steps of an mbx_step action: the reference's skip_step */
#define MBX_SYM_NFEAT      9
#define MBX_SYM_TOK_ADD    0
#define MBX_SYM_TOK_MUL    1
#define MBX_SYM_TOK_NEG    2
#define MBX_SYM_TOK_CM1    3
#define MBX_SYM_TOK_C0     4
#define MBX_SYM_TOK_X      5
#define MBX_SYM_TOK_GB     6
#define MBX_SYM_TOK_GW     7
#define MBX_SYM_TOK_DX     8
#define MBX_SYM_TOK_RANDX  9
#define MBX_SYM_TOK_PB     10
#define MBX_SYMBOL_TAPE_POS(NP, D)        ((int64_t)0)
#define MBX_SYMBOL_TAPE_NOISE_INIT(NP, D) ((int64_t)(NP) * (D))
#define MBX_SYMBOL_TAPE_SUB(NP, D, S)     ((int64_t)(NP) * (D) + 3 * (int64_t)(NP) + (int64_t)(S) * (MBX_SYM_RANDX_MAX + 3) * (int64_t)(NP))
#define MBX_SYMBOL_SUB_IDX(NP, D)         ((int64_t)0)
#define MBX_SYMBOL_SUB_NOISE(NP, D)       ((int64_t)MBX_SYM_RANDX_MAX * (NP))
#define MBX_SYMBOL_TAPE_STRIDE(NP, D)     MBX_SYMBOL_TAPE_SUB(NP, D, MBX_SYM_SUB_MAX)
#define MBX_SYMBOL_ST_X(NP, D)            ((int64_t)0)
#define MBX_SYMBOL_ST_PBPOS(NP, D)        ((int64_t)(NP) * (D))
#define MBX_SYMBOL_ST_DX(NP, D)           (2 * (int64_t)(NP) * (D))
#define MBX_SYMBOL_ST_COST(NP, D)         (3 * (int64_t)(NP) * (D))
#define MBX_SYMBOL_ST_PBEST(NP, D)        (3 * (int64_t)(NP) * (D) + (NP))
#define MBX_SYMBOL_ST_GBPOS(NP, D)        (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP))
#define MBX_SYMBOL_ST_GWPOS(NP, D)        (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP) + (D))
#define MBX_SYMBOL_ST_CBPOS(NP, D)        (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP) + 2 * (int64_t)(D))
#define MBX_SYMBOL_ST_FEAT(NP, D)         (3 * (int64_t)(NP) * (D) + 2 * (int64_t)(NP) + 3 * (int64_t)(D))
#define MBX_SYMBOL_ST_SCALARS(NP, D)      (MBX_SYMBOL_ST_FEAT(NP, D) + 10)
#define MBX_SYMBOL_ST_IDX(NP, D, NLOG)    (MBX_SYMBOL_ST_SCALARS(NP, D) + MBX_NSCALAR + (int64_t)(NLOG) + 1)      /* in doubles; the region holds bytes */
#define MBX_SYMBOL_STATE_DOUBLES(NP, D, NLOG) (MBX_SYMBOL_ST_IDX(NP, D, NLOG) + (int64_t)MBX_SYM_SUB_MAX * MBX_SYM_RANDX_MAX * (NP) / 8 + 1)
#define MBX_SC_SYM_SUB       9    /* sub-steps done of the action in progress (0 between actions) */
#define MBX_SC_SYM_GWORST    10   /* gworst_cost: the worst cost ever seen (strict >) */
#define MBX_SC_SYM_CBEST     11   /* cbest_cost: the best of the last evaluated generation */
#define MBX_SC_SYM_CBEST_IDX 12
#define MBX_SC_SYM_STAG      13   /* stag_count */
#define MBX_SC_SYM_PRE_GBEST 14   /* gbest at the start of the last action */
#define MBX_SC_SYM_INIT_COST 15   /* the best cost of the initial population */
#define MBX_SITE_SYM_IDX     84u

#define MBX_PHILOX_M0 0xD2511F53u
#define MBX_PHILOX_M1 0xCD9E8D57u
#define MBX_PHILOX_W0 0x9E3779B9u
#define MBX_PHILOX_W1 0xBB67AE85u

#endif /* MBX_LAYOUT_H */
