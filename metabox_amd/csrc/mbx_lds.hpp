// mbx_lds.hpp — the dynamic-LDS map of every kernel family, free of kernels.
//
// Each family has ONE description of its layout: a walk  template <class C> XLds x_layout(C& c, ...)  that asks a cursor for every array in
// order, `c.take<T>(doubles)`.  Two cursors run the same walk:
//   * LdsSize only adds: x_lds_doubles(...) is where the walk ends -- the byte count the host passes to the launch;
//   * LdsCarve bumps a pointer: x_carve(smem, ...) is what the kernel indexes.
// So a size and its pointers cannot disagree.  All extents are in doubles; the base is 16-byte aligned and every extent is even, so every array
// starts 16-byte aligned.  Arrays that share storage (an area that is dead while another phase uses it) are walks too: a second cursor starts
// at the same place, and the enclosing take asks for where it ends, or for the longest of the alternatives.  (Eight families keep a carve written out by
// hand beside their walk -- dq, dd, jd, md, sd, nr, ql, rp: their kernels measured slower through the walk.  Their
// sizes are the walks', and tests/lds_sizes_main.hip holds every hand-written pointer to the walk's.  k_rs_population and k_eval carve inline in their kernels, as
// they always did; only their sizes come from rs_layout / ev_layout.)
#pragma once
#include "mbx_device.hpp"

namespace mbx {

__host__ __device__ inline int64_t align2(int64_t n) { return (n + 1) & ~(int64_t)1; }

struct LdsSize {
    int64_t n = 0;
    template <class T = double> __host__ __device__ T* take(int64_t doubles) { n += doubles; return nullptr; }
};

struct LdsCarve {
    double* p;
    template <class T = double> __host__ __device__ __forceinline__ T* take(int64_t doubles) { T* r = reinterpret_cast<T*>(p); p += doubles; return r; }
};

#define MBX_LDS_WALK template <class C> __host__ __device__ __forceinline__

// four waves per SIMD: left alone the compiler takes 126-160 VGPRs for the multi-step / sweep kernels (three resident workgroups per CU
// although the LDS would hold five); capped at 128 they spill little or nothing (QLPSO rollout 82 -> 69 us, RL-PSO rollout 60 -> 53 us per step)
#ifndef MBX_N4_WAVES
#define MBX_N4_WAVES __attribute__((amdgpu_waves_per_eu(4)))
#endif

// ------------------------------------------------------------------------------------------------ the evaluator's share
// the evaluator's scratch Z for `rows` rows: a double per element, and never less than two per thread, which the block reductions use
__host__ __device__ inline int64_t eval_z_doubles(int rows, int D)
{
    const int64_t NE = align2((int64_t)rows * D);
    return align2(NE > 2 * kThreads ? NE : 2 * kThreads);
}

// the rows and the scratch of one evaluation of `rows` rows: X | T | Z
MBX_LDS_WALK void lds_eval_rows(C& c, int rows, int D, double*& X, double*& T, double*& Z)
{
    X = c.take(align2((int64_t)rows * D));
    T = c.take(eval_t_doubles(rows, D));
    Z = c.take(eval_z_doubles(rows, D));
}

// the problem's constants: the two D x D maps (none when the kernel reads them from global memory) and the four D-vectors
MBX_LDS_WALK void lds_eval_consts(C& c, int D, bool maps, double*& M1T, double*& M2T, double*& DSH, double*& V0, double*& V1, double*& V2)
{
    const int64_t DD = maps ? align2((int64_t)D * D) : 0, DV = align2(D);
    M1T = c.take(DD);  M2T = c.take(DD);
    DSH = c.take(DV);  V0 = c.take(DV);  V1 = c.take(DV);  V2 = c.take(DV);
}

// X | T | Z | M1T | M2T | DSH | V0 | V1 | V2: what most families begin with
MBX_LDS_WALK void lds_eval_prefix(C& c, int rows, int D, double*& X, double*& T, double*& Z, double*& M1T, double*& M2T, double*& DSH, double*& V0,
                                  double*& V1, double*& V2)
{
    lds_eval_rows(c, rows, D, X, T, Z);
    lds_eval_consts(c, D, true, M1T, M2T, DSH, V0, V1, V2);
}

// ------------------------------------------------------------------------------------------------ RLEPSO (mbx_rlepso.hpp)
struct RlLds {
    double *PB, *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *PBC, *NC, *PNI, *CMUT, *R1, *R2, *GB, *COEF, *RED;
    int *IMPR, *MASK, *RANK;
    // KB (NE bytes): rank of the FDR exemplar of every (rank, dimension), carved out of the part of Z that R1 / R2 / COEF leave free
    // (all dead before the evaluator first writes Z)
    uint8_t* KB;
    // FL (one uint16 per work item of the FDR pass) / FLN: the items whose scan met a near-tie, appended by their owners and settled wave-cooperatively (fdr_settle); same
    // free part of Z, behind KB
    uint16_t* FL;
    int* FLN;
    // NCS [NP]: the cost column the FDR scan reads -- NC with the rows that are bitwise copies of the row one rank up (same cost, same position: particles sitting on
    // the same corner of the box) replaced by a huge value, so that the scan never takes them and never mistakes them for near-ties (rl_mark_copies); same free part of Z
    double* NCS;
    int zd;                       // doubles of Z (rl_z_doubles)
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC, zd}; }
};

// the move phase's tables, which live in Z (all last read in the move phase; Z is first written by the evaluator):
// R1 | R2 (per-particle draws) | COEF (6 coefficients for each of up to 16 groups) | NCS | KB (NE bytes, padded to 16) | FLN + pad (16 bytes) | FL (up to NE uint16)
MBX_LDS_WALK void rl_move_layout(C& c, RlLds& L, int NP, int D)
{
    const int64_t NE = (int64_t)NP * D, P = align2(NP);
    L.R1 = c.take(P);  L.R2 = c.take(P);  L.COEF = c.take(96);  L.NCS = c.take(P);
    L.KB = c.template take<uint8_t>((NE + 15) / 16 * 2);  L.FLN = c.template take<int>(2);  L.FL = c.template take<uint16_t>((2 * NE + 7) / 8);
}

// evaluator scratch Z: the longest of what its users need
__host__ __device__ inline int64_t rl_z_doubles(int NP, int D)
{
    RlLds L; LdsSize move;
    rl_move_layout(move, L, NP, D);
    int64_t need = move.n;
    if (need < 2 * kThreads) need = 2 * kThreads;               // two per thread for the block reductions
    if (D == 12 && need < 4 * 4 * 100) need = 4 * 4 * 100;      // protein docking (D = 12, 100 atoms): one 32-byte-per-atom table per wave of a 256-thread workgroup (eval_rows_protein)
    const int64_t NE = align2((int64_t)NP * D);                 // the evaluator's n*D
    return align2(NE > need ? NE : need);
}

// PB (aliased by the evaluator's scratch T once the velocity phase is over, see rl_commit) | X | Z | M1T, M2T (none where the kernels read the maps
// from global memory) | DSH, V0, V1, V2 | PBC, NC, PNI, CMUT | GB | RED | three int arrays  (29.8 KB at NP = 100, D = 10: five workgroups per CU)
MBX_LDS_WALK RlLds rl_layout(C& c, int NP, int D, bool maps)
{
    const int64_t P = align2(NP), PI = align2((P + 1) / 2), SC = rl_z_doubles(NP, D);
    RlLds L;
    L.PB = L.T = c.take(eval_t_doubles(NP, D));
    L.X = c.take(align2((int64_t)NP * D));
    C move = c;
    rl_move_layout(move, L, NP, D);
    L.Z = c.take(SC);  L.zd = (int)SC;
    lds_eval_consts(c, D, maps, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.PBC = c.take(P);  L.NC = c.take(P);  L.PNI = c.take(P);  L.CMUT = c.take(P);
    L.GB = c.take(align2(D));  L.RED = c.take(16);
    L.IMPR = c.template take<int>(PI);  L.MASK = c.template take<int>(PI);  L.RANK = c.template take<int>(PI);
    return L;
}
__host__ __device__ inline int64_t rl_lds_doubles(int NP, int D, bool maps = true) { LdsSize c; rl_layout(c, NP, D, maps); return c.n; }
__device__ __forceinline__ RlLds rl_carve(double* base, int NP, int D, bool maps = true) { LdsCarve c{base}; return rl_layout(c, NP, D, maps); }

// ------------------------------------------------------------------------------------------------ LDE step kernels (mbx_lde.hpp)
struct LdeLds {
    double *P, *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *FIT, *NC, *SF, *CR, *SORTED, *RED, *HS;
    int *PIDX, *R0, *R1, *JR, *HIST;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

MBX_LDS_WALK LdeLds lde_layout(C& c, int NP, int D, bool maps)
{
    const int64_t NE = align2((int64_t)NP * D), P = align2(NP), PI = align2((P + 1) / 2), TS = eval_t_doubles(NP, D), SC = eval_z_doubles(NP, D);
    LdeLds L;
    // P (the parents) is dead between the mutation and the selection, exactly while the evaluator needs its scratch T: they share
    // storage and the unchanged parents are re-read from HBM after the evaluation (12 KB less LDS at NP = 50, D = 30: three resident
    // workgroups per CU instead of two).
    L.P = L.T = c.take(NE > TS ? NE : TS);
    L.X = c.take(NE);
    C rates = c;                                                 // scale factors / crossover rates: last read by the mutation, Z first written by the evaluator
    L.SF = rates.take(P);  L.CR = rates.take(P);
    L.Z = c.take(SC);                                            // SC >= 2 * kThreads >= 2 P: the rates fit
    lds_eval_consts(c, D, maps, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.FIT = c.take(P);
    L.NC = L.SORTED = c.take(P);                                 // the trials' costs are dead once the selection is done
    L.RED = c.take(16);  L.HS = c.take(8);
    L.PIDX = c.template take<int>(PI);  L.R0 = c.template take<int>(PI);  L.R1 = c.template take<int>(PI);  L.JR = c.template take<int>(PI);
    L.HIST = c.template take<int>(8);
    return L;
}
__host__ __device__ inline int64_t lde_lds_doubles(int NP, int D, bool maps = true) { LdsSize c; lde_layout(c, NP, D, maps); return c.n; }
__device__ __forceinline__ LdeLds lde_carve(double* base, int NP, int D, bool maps = true) { LdsCarve c{base}; return lde_layout(c, NP, D, maps); }

// ------------------------------------------------------------------------------------------------ LDE resident kernel (mbx_lde_run.hpp)
struct LdeRunLds {
    double *P, *TB, *TB2, *FIT, *A1, *A2, *FEAT, *HS, *RED, *SCAL, *DSH;
    float *ACT, *HC;
    uint8_t *RK, *ORDER;         // rank of a physical row / row at a rank (NP <= 255)
    int *ACC, *HIST, *FLAG;      // ACC: the ranking's per-row counters
};

// LDS is allocated in 1280-byte granules: 3 workgroups per CU need <= 53 760 B each (pop 100: 52 768 B), 6 need <= 26 880 B (pop 50: 26 880 B)
MBX_LDS_WALK LdeRunLds lde_run_layout(C& c, int NP, int D, int H, bool two)
{
    const int64_t NE = align2((int64_t)NP * D), P = align2(NP);
    LdeRunLds L;
    L.P = c.take(NE);  L.TB = c.take(NE);
    L.TB2 = two ? c.take(NE) : nullptr;                          // second tile array (kinds 3, 4, 5, 15, 20, 24)
    L.FIT = c.take(P);
    L.A1 = c.take(P);            // SORTED (from the ranking to the next row sums) | Gallagher: best key per row
    L.FEAT = L.A2 = c.take(align2(NP + 2 * MBX_LDE_BINS));       // features; dead between the policy's input staging and the next feature phase, where
                                 // the objective uses the storage: F0 (step ellipsoid: |z_hat_0|) | Gallagher: winning peak per row
    L.HS = c.take(8);  L.RED = c.take(8);  L.SCAL = c.take(8);
    L.ACT = c.template take<float>(P);                           // 2 NP floats
    L.HC = c.template take<float>(align2(H));                    // h | c
    L.ACC = c.template take<int>(align2((P + 1) / 2));
    L.RK = c.template take<uint8_t>(align2((P + 7) / 8));  L.ORDER = c.template take<uint8_t>(align2((P + 7) / 8));
    L.HIST = c.template take<int>(4);                            // [5] bin counts, [6] the done flag
    L.FLAG = L.HIST + 6;
    L.DSH = c.take(align2(D));                                   // the problem's shift vector (0 where the objective has none)
    return L;
}
__host__ __device__ inline int64_t lde_run_lds_doubles(int NP, int D, int H, bool two) { LdsSize c; lde_run_layout(c, NP, D, H, two); return c.n; }
__device__ __forceinline__ LdeRunLds lde_run_carve(double* base, int NP, int D, int H, bool two) { LdsCarve c{base}; return lde_run_layout(c, NP, D, H, two); }

// ------------------------------------------------------------------------------------------------ DE-DDQN (mbx_ddqn.hpp)
constexpr int kDqRec = 820;
struct DqLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *COST, *REC, *FEAT, *RED, *MISC;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
    // REC: N_tot[40] | N_succ[160] | OM_sum[160] | OM_max[160] | OM_W[300]
    __device__ __forceinline__ double* ntot() const { return REC; }
    __device__ __forceinline__ double* nsucc() const { return REC + 40; }
    __device__ __forceinline__ double* omsum() const { return REC + 200; }
    __device__ __forceinline__ double* ommax() const { return REC + 360; }
    __device__ __forceinline__ double* omw() const { return REC + 520; }
};

// rows: how many candidates the evaluator sees at once -- NP in k_dq_reset, ONE in k_dq_step (a step evaluates a single trial vector:
// 17.9 KB instead of 40.9 KB at NP = 100, D = 12, so the register budget, not the LDS, decides how many workgroups share a CU)
MBX_LDS_WALK DqLds dq_layout(C& c, int rows, int NP, int D)
{
    const int64_t P = align2(NP);
    DqLds L;
    lds_eval_prefix(c, rows, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(P);  L.COST = c.take(P);  L.REC = c.take(kDqRec);  L.FEAT = c.take(100);  L.RED = c.take(16);
    L.MISC = c.take(16 + 2 * align2(D));                         // the step's indices and scalars [8] | prebest position | gbest position | 8 spare
    return L;
}
__host__ __device__ inline int64_t dq_lds_doubles(int rows, int NP, int D) { LdsSize c; dq_layout(c, rows, NP, D); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ DqLds dq_carve(double* base, int rows, int NP, int D)
{
    const int64_t NE = align2((int64_t)rows * D), SC = eval_z_doubles(rows, D), DD = align2((int64_t)D * D), P = align2(NP);
    DqLds L;
    double* p = base;
    L.X = p; p += NE;  L.T = p; p += eval_t_doubles(rows, D);  L.Z = p; p += SC;  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);
    L.NC = p; p += P;  L.COST = p; p += P;  L.REC = p; p += kDqRec;  L.FEAT = p; p += 100;  L.RED = p; p += 16;  L.MISC = p;
    return L;
}

// ------------------------------------------------------------------------------------------------ DEDQN (mbx_dedqn.hpp)
struct DdLds {
    double *POP, *T, *Z, *M1T, *M2T, *DSH, *V0, *V1, *V2, *TRIAL, *GB, *COST, *SURV, *SCOST, *DIST, *SORTED, *DIFF, *RED, *SC, *FEAT, *HS;
    int *CNT, *IR;
    __device__ __forceinline__ EvalLds eval(const double* x, double* f) const { return EvalLds{x, Z, T, M1T, M2T, DSH, V0, V1, V2, f}; }
};

// POP, Z (the evaluator's scratch, then the walk) and T: NP * D each -- 8 KB at NP = 100 / D = 10, 40 KB at NP = 128 / D = 40 (146 KB in all there)
MBX_LDS_WALK DdLds dd_layout(C& c, int NP, int D)
{
    const int64_t P = align2(NP), DV = align2(D);
    DdLds L;
    lds_eval_prefix(c, NP, D, L.POP, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.TRIAL = c.take(DV);  L.GB = c.take(DV);
    L.COST = c.take(P);  L.SURV = c.take(P);  L.SCOST = c.take(P);  L.DIST = c.take(P);  L.SORTED = c.take(P);  L.DIFF = c.take(P);
    L.RED = c.take(32);  L.SC = c.take(MBX_NSCALAR);  L.FEAT = c.take(MBX_DEDQN_FEAT_SLOTS);  L.HS = c.take(10);
    L.CNT = c.template take<int>(64);                            // two waves x (9 levels x 6 classes + the descent count)
    L.IR = c.template take<int>(4);
    return L;
}
__host__ __device__ inline int64_t dd_lds_doubles(int NP, int D) { LdsSize c; dd_layout(c, NP, D); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ DdLds dd_carve(double* base, int NP, int D)
{
    const int64_t NE = align2((int64_t)NP * D), ZS = eval_z_doubles(NP, D), DD = align2((int64_t)D * D), P = align2(NP);
    DdLds L;
    double* p = base;
    L.POP = p; p += NE;  L.T = p; p += eval_t_doubles(NP, D);  L.Z = p; p += ZS;  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);
    L.TRIAL = p; p += align2(D);  L.GB = p; p += align2(D);
    L.COST = p; p += P;  L.SURV = p; p += P;  L.SCOST = p; p += P;  L.DIST = p; p += P;  L.SORTED = p; p += P;  L.DIFF = p; p += P;
    L.RED = p; p += 32;  L.SC = p; p += MBX_NSCALAR;  L.FEAT = p; p += MBX_DEDQN_FEAT_SLOTS;  L.HS = p; p += 10;
    L.CNT = (int*)p; p += 64;                                       // two waves x (9 levels x 6 classes + the descent count)
    L.IR = (int*)p;
    return L;
}

// ------------------------------------------------------------------------------------------------ GLEET (mbx_gleet.hpp)
struct GlLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *GB, *K1, *K2, *GF;
    int* IMPR;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

MBX_LDS_WALK GlLds gl_layout(C& c, int NP, int D)
{
    const int64_t P = align2(NP);
    GlLds L;
    lds_eval_prefix(c, NP, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.GB = c.take(align2(D));
    L.NC = c.take(P);  L.K1 = c.take(P);  L.K2 = c.take(P);  L.RED = c.take(16);  L.GF = c.take(10);
    L.IMPR = c.template take<int>(align2((P + 1) / 2));
    return L;
}
__host__ __device__ inline int64_t gl_lds_doubles(int NP, int D) { LdsSize c; gl_layout(c, NP, D); return c.n; }
__device__ __forceinline__ GlLds gl_carve(double* base, int NP, int D) { LdsCarve c{base}; return gl_layout(c, NP, D); }

// The resident rollout (mbx_gleet_run.hpp): the generation's layout, then the actor's.  Its keys and values (K | V, [NP][16] float32 each: 16 NP doubles) are
// only alive while the evaluator's scratch T | Z is dead, and lie there wherever that is long enough (D >= 8, or a small swarm); otherwise they get an area
// of their own behind everything else.  PRED: the actor's block sums, one float per wave.
struct GlrLds {
    GlLds g;
    float *KL, *VL, *PRED;
};

__host__ __device__ inline int64_t glr_kv_doubles(int NP) { return 16 * (int64_t)NP; }
__host__ __device__ inline bool glr_kv_in_scratch(int NP, int D) { return glr_kv_doubles(NP) <= eval_t_doubles(NP, D) + eval_z_doubles(NP, D); }

MBX_LDS_WALK GlrLds glr_layout(C& c, int NP, int D)
{
    GlrLds L;
    L.g = gl_layout(c, NP, D);
    L.PRED = c.template take<float>(2);
    L.KL = glr_kv_in_scratch(NP, D) ? reinterpret_cast<float*>(L.g.T) : c.template take<float>(glr_kv_doubles(NP));      // T | Z are contiguous (lds_eval_rows)
    L.VL = L.KL + 16 * NP;
    return L;
}
__host__ __device__ inline int64_t glr_lds_doubles(int NP, int D) { LdsSize c; glr_layout(c, NP, D); return c.n; }
__device__ __forceinline__ GlrLds glr_carve(double* base, int NP, int D) { LdsCarve c{base}; return glr_layout(c, NP, D); }

// ------------------------------------------------------------------------------------------------ GL-PSO (mbx_glpso.hpp)
struct GpLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *GB, *PBC, *EXC, *STAG, *RED;
    int* FLAG;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

// X: evaluation rows (the swarm, then the new exemplars); Z: evaluator scratch, holds pbest_pos / the exemplars between the evaluations
MBX_LDS_WALK GpLds gp_layout(C& c, int NP, int D)
{
    const int64_t P = align2(NP);
    GpLds L;
    lds_eval_prefix(c, NP, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.GB = c.take(align2(D));
    L.NC = c.take(P);  L.PBC = c.take(P);  L.EXC = c.take(P);  L.STAG = c.take(P);  L.RED = c.take(16);
    L.FLAG = c.template take<int>(align2((P + 1) / 2));
    return L;
}
__host__ __device__ inline int64_t gp_lds_doubles(int NP, int D) { LdsSize c; gp_layout(c, NP, D); return c.n; }
__device__ __forceinline__ GpLds gp_carve(double* base, int NP, int D) { LdsCarve c{base}; return gp_layout(c, NP, D); }

// ------------------------------------------------------------------------------------------------ JDE21 (mbx_jde21.hpp)
constexpr int kJdS = MBX_JDE21_SNP;
// LDS row stride of the staged population and of the trials.  The lanes of a wave read 16 consecutive rows at once (8 bytes each): with a
// stride of D doubles they hit distinct banks unless D is a multiple of 4 (D = 12: 2-way, D = 40: 4-way conflicts), where one double of
// padding makes the stride odd.
__host__ __device__ inline int jd_stride(int D) { return D % 4 == 0 ? D + 1 : D; }
__host__ __device__ inline int64_t jd_stage_doubles(int NP, int D) { return align2((int64_t)(NP - kJdS) * jd_stride(D)); }
// LDS of one evaluation chunk of ch rows: X | T | Z  (written out: jd_chunk runs in the kernels)
__host__ __device__ inline int64_t jd_ev_doubles(int ch, int D)
{
    const int64_t ne = (int64_t)ch * D;
    return align2(ne) + eval_t_doubles(ch, D) + align2(ne > 2 * kThreads ? ne : 2 * kThreads);
}
// rows per evaluation chunk: at most 80, at least 54 (the big pass in three chunks), what fits the staging area of the big population between
__host__ __device__ inline int jd_chunk(int NP, int D)
{
    int ch = 80;
    while (ch > 54 && jd_ev_doubles(ch, D) > jd_stage_doubles(NP, D)) --ch;
    return ch;
}

// the staging area of the big population's trials | one evaluation chunk, whichever is longer
__host__ __device__ inline int64_t jd_ev_area(int NP, int D)
{
    const int64_t a = jd_stage_doubles(NP, D), b = jd_ev_doubles(jd_chunk(NP, D), D);
    return a > b ? a : b;
}

struct JdLds {
    double *UP, *EV, *M1T, *M2T, *DSH, *V0, *V1, *V2, *SP, *COST, *FF, *CR, *TC, *TF, *TCR, *RED;
    double* ACC;           // shares TC's memory: the selection reads the trial costs before its barrier and writes ACC after it
    int *R1, *R2, *R3, *JR, *CID, *WIN;
    // the evaluator's view of the staging area for a chunk of ch rows, costs into f
    __device__ __forceinline__ EvalLds eval(int ch, int D, double* f) const
    {
        double* T = EV + align2((int64_t)ch * D);
        return EvalLds{EV, T + eval_t_doubles(ch, D), T, M1T, M2T, DSH, V0, V1, V2, f};
    }
};

MBX_LDS_WALK JdLds jd_layout(C& c, int NP, int D)
{
    const int64_t P = align2(NP), PI = align2((P + 1) / 2);
    JdLds L;
    L.UP = c.take(jd_stage_doubles(NP, D));
    L.EV = c.take(jd_ev_area(NP, D));
    lds_eval_consts(c, D, true, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.SP = c.take(align2(kJdS * D));
    L.COST = c.take(P);  L.FF = c.take(P);  L.CR = c.take(P);  L.TC = L.ACC = c.take(P);  L.TF = c.take(P);  L.TCR = c.take(P);
    L.RED = c.take(16);
    L.R1 = c.template take<int>(PI);  L.R2 = c.template take<int>(PI);  L.R3 = c.template take<int>(PI);
    L.JR = c.template take<int>(PI);  L.CID = c.template take<int>(PI);  L.WIN = c.template take<int>(PI);
    return L;
}
__host__ __device__ inline int64_t jd_lds_doubles(int NP, int D) { LdsSize c; jd_layout(c, NP, D); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ JdLds jd_carve(double* base, int NP, int D)
{
    const int64_t DD = align2((int64_t)D * D), P = align2(NP), PI = align2((P + 1) / 2);
    JdLds L;
    double* p = base;
    L.UP = p; p += jd_stage_doubles(NP, D);  L.EV = p; p += jd_ev_area(NP, D);  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);  L.SP = p; p += align2(kJdS * D);
    L.COST = p; p += P;  L.FF = p; p += P;  L.CR = p; p += P;  L.TC = p; L.ACC = p; p += P;  L.TF = p; p += P;  L.TCR = p; p += P;
    L.RED = p; p += 16;
    L.R1 = reinterpret_cast<int*>(p); p += PI;  L.R2 = reinterpret_cast<int*>(p); p += PI;  L.R3 = reinterpret_cast<int*>(p); p += PI;
    L.JR = reinterpret_cast<int*>(p); p += PI;  L.CID = reinterpret_cast<int*>(p); p += PI;  L.WIN = reinterpret_cast<int*>(p);
    return L;
}

// ------------------------------------------------------------------------------------------------ the sorted-DE kernels (mbx_depop.hpp: MadDE, NL_SHADE_LBC, RL-HPSDE)
// rows per evaluation chunk
__host__ __device__ inline int md_chunk(int D) { return D <= 12 ? 128 : D <= 30 ? 96 : 64; }
__host__ __device__ inline int md_pad(int n) { int p = 2; while (p < n) p <<= 1; return p; }

struct MdLds {
    double *EV, *M1T, *M2T, *DSH, *V0, *V1, *V2, *TC, *RED, *VEC, *KEY;
    int *CNT, *LIST, *WIN, *IDX;
    uint8_t* MU;
    __device__ __forceinline__ EvalLds eval(int ch, int D, double* f) const
    {
#ifdef MBX_MD_WALK_CARVE
        LdsCarve c{EV};
        double *X, *T, *Z;
        lds_eval_rows(c, ch, D, X, T, Z);
        return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, f};
#else
        double* T = EV + align2((int64_t)ch * D);
        return EvalLds{EV, T + eval_t_doubles(ch, D), T, M1T, M2T, DSH, V0, V1, V2, f};
#endif
    }
};

// the area the phases of an update share, three walks from one place: evaluation chunk | archive winners (int) + compacted vector | sort keys + rows (int)
MBX_LDS_WALK void md_work_layout(C& ev, C& arc, C& sort, MdLds& L, int NP, int D)
{
    double *T, *Z;
    lds_eval_rows(ev, md_chunk(D), D, L.EV, T, Z);
    L.WIN = arc.template take<int>(align2((MBX_MADDE_ARC(NP) + 1) / 2));  L.VEC = arc.take(align2(NP));
    L.KEY = sort.take(md_pad(NP));  L.IDX = sort.template take<int>(align2(md_pad(NP) / 2));
}
__host__ __device__ inline int64_t md_work_doubles(int NP, int D)
{
    MdLds L; LdsSize a, b, c;
    md_work_layout(a, b, c, L, NP, D);
    return a.n > b.n ? (a.n > c.n ? a.n : c.n) : (b.n > c.n ? b.n : c.n);
}

MBX_LDS_WALK MdLds md_layout(C& c, int NP, int D)
{
    MdLds L;
    C ev = c, arc = c, sort = c;
    md_work_layout(ev, arc, sort, L, NP, D);
    c.take(md_work_doubles(NP, D));
    lds_eval_consts(c, D, true, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.TC = c.take(align2(md_chunk(D)));  L.RED = c.take(16);
    L.CNT = c.template take<int>(2 * kThreads);  L.LIST = c.template take<int>(align2((NP + 1) / 2));  L.MU = c.template take<uint8_t>(align2((NP + 7) / 8));
    return L;
}
__host__ __device__ inline int64_t md_lds_doubles(int NP, int D) { LdsSize c; md_layout(c, NP, D); return c.n; }
// The carve-up and MdLds::eval stay written out by hand for time: through the walk k_nlshade_step measured 2.1 % slower (docs/EXPERIMENTS.md "One walk per LDS
// layout").  -DMBX_MD_WALK_CARVE (the Makefile's EXTRA) builds both through md_layout / lds_eval_rows instead: same pointers, other register allocation.  That form
// once made k_nlshade_run write a gbest with the bit pattern of two small ints from the second update of a launch on; the cause was the compiler's, not the layout's
// (register copies placed ahead of the exec restore of a join block: docs/EXPERIMENTS.md "NL_SHADE_LBC: the multi-update garbage"), and the multi-update tests of
// tests/test_nlshade.py are what holds either form to the one-update launches.  The size above is the walk's, and tests/lds_sizes_main.hip holds these pointers to
// the walk's over its grid.
__host__ __device__ inline int64_t md_ev_doubles(int ch, int D)
{
    const int64_t ne = (int64_t)ch * D;
    return align2(ne) + eval_t_doubles(ch, D) + align2(ne > 2 * kThreads ? ne : 2 * kThreads);
}
__host__ __device__ inline int64_t md_win_doubles(int NP) { return align2((MBX_MADDE_ARC(NP) + 1) / 2); }
__host__ __device__ inline int64_t md_work_hand_doubles(int NP, int D)
{
    const int64_t a = md_ev_doubles(md_chunk(D), D), b = md_win_doubles(NP) + align2(NP), c = md_pad(NP) + align2(md_pad(NP) / 2);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}
// where the carve ends (RL-HPSDE's kernels find their FT there): md_lds_doubles in the same arithmetic
__host__ __device__ inline int64_t md_lds_hand_doubles(int NP, int D)
{
    const int64_t DD = align2((int64_t)D * D);
    return md_work_hand_doubles(NP, D) + 2 * DD + 4 * align2(D) + align2(md_chunk(D)) + 16 + 2 * kThreads + align2((NP + 1) / 2) + align2((NP + 7) / 8);
}
__host__ __device__ __forceinline__ MdLds md_carve(double* base, int NP, int D)
{
#ifdef MBX_MD_WALK_CARVE
    LdsCarve c{base};
    return md_layout(c, NP, D);
#else
    const int64_t DD = align2((int64_t)D * D);
    MdLds L;
    double* p = base;
    L.EV = p; L.WIN = reinterpret_cast<int*>(p); L.VEC = p + md_win_doubles(NP); L.KEY = p; L.IDX = reinterpret_cast<int*>(p + md_pad(NP));
    p += md_work_hand_doubles(NP, D);
    L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);
    L.TC = p; p += align2(md_chunk(D));  L.RED = p; p += 16;
    L.CNT = reinterpret_cast<int*>(p); p += 2 * kThreads;
    L.LIST = reinterpret_cast<int*>(p); p += align2((NP + 1) / 2);
    L.MU = reinterpret_cast<uint8_t*>(p);
    return L;
#endif
}

__host__ __device__ inline int64_t nl_lds_doubles(int N0, int D) { return md_lds_doubles(N0, D); }

constexpr int kHpFeatDoubles = 752;     // walk costs [202] | distances [200] | differences [202] | entropies [12] | counts: 4 waves x 64 ints
// RL-HPSDE: the shared layout, then the landscape walk's FT, which its kernels find at smem + md_lds_hand_doubles
__host__ __device__ inline int64_t hp_lds_doubles(int NP, int D) { LdsSize c; md_layout(c, NP, D); c.take(kHpFeatDoubles); return c.n; }

// ------------------------------------------------------------------------------------------------ sDMS_PSO (mbx_sdmspso.hpp)
struct SdLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *GB, *NC, *PBC, *R1, *R2, *LBP, *LBC, *IWT, *SUC, *RED;
    int *FLAG, *PERM, *LBI, *SWF;
    uint32_t* KEY;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

MBX_LDS_WALK SdLds sd_layout(C& c, int NP, int D)
{
    const int64_t P = align2(NP), NSA = align2(MBX_SDMS_NS);
    SdLds L;
    lds_eval_prefix(c, NP, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.GB = c.take(align2(D));
    L.NC = c.take(P);  L.PBC = c.take(P);  L.R1 = c.take(P);  L.R2 = c.take(P);  L.LBP = c.take(align2((int64_t)MBX_SDMS_NS * D));
    L.LBC = c.take(NSA);  L.IWT = c.take(NSA);  L.SUC = c.take(NSA);  L.RED = c.take(16);
    // P and NSA are even: every int array is a whole number of doubles
    L.FLAG = c.template take<int>(P / 2);  L.PERM = c.template take<int>(P / 2);  L.KEY = c.template take<uint32_t>(P / 2);
    L.LBI = c.template take<int>(NSA / 2);  L.SWF = c.template take<int>(NSA / 2);
    c.take((3 * P / 2 + NSA) & 1);                               // keeps the total even
    return L;
}
__host__ __device__ inline int64_t sd_lds_doubles(int NP, int D) { LdsSize c; sd_layout(c, NP, D); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ SdLds sd_carve(double* base, int NP, int D)
{
    const int64_t NE = align2((int64_t)NP * D), SC = eval_z_doubles(NP, D), DD = align2((int64_t)D * D), P = align2(NP);
    const int64_t NSA = align2(MBX_SDMS_NS);
    SdLds L;
    double* p = base;
    L.X = p; p += NE;  L.T = p; p += eval_t_doubles(NP, D);  L.Z = p; p += SC;  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);  L.GB = p; p += align2(D);
    L.NC = p; p += P;  L.PBC = p; p += P;  L.R1 = p; p += P;  L.R2 = p; p += P;  L.LBP = p; p += align2((int64_t)MBX_SDMS_NS * D);
    L.LBC = p; p += NSA;  L.IWT = p; p += NSA;  L.SUC = p; p += NSA;  L.RED = p; p += 16;
    int* q = reinterpret_cast<int*>(p);
    L.FLAG = q; q += P;  L.PERM = q; q += P;  L.KEY = reinterpret_cast<uint32_t*>(q); q += P;  L.LBI = q; q += NSA;  L.SWF = q;
    return L;
}

// ------------------------------------------------------------------------------------------------ NRLPSO (mbx_nrlpso.hpp)
constexpr int kNrK = MBX_NRLPSO_K;
__host__ __device__ inline int nr_stride(int NP) { return NP | 1; }

struct NrLds {
    double *X, *T, *Z, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *POP, *PB, *COST, *PBCOST, *STAG, *SS, *DIST, *TMP, *GB, *SC, *DG, *DM;
    int *PNI, *GNI;
    __device__ __forceinline__ EvalLds eval(const double* x, double* f) const { return EvalLds{x, Z, T, M1T, M2T, DSH, V0, V1, V2, f}; }
};

// rows = evaluation rows of the launch: NP for the reset (its X doubles as the population), 1 for a step (step = true: the resident arrays,
// and with cached = true the distance matrix: 80.8 KB at NP = 100; 132 KB at NP = 128, which fits the 160 KB up to D = 7 only)
MBX_LDS_WALK NrLds nr_layout(C& c, int rows, int NP, int D, bool step, bool cached)
{
    const int64_t P = align2(NP), PE = align2((int64_t)NP * D);
    NrLds L{};
    lds_eval_prefix(c, rows, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(align2(rows));  L.RED = c.take(32);  L.COST = c.take(P);
    L.POP = L.X;
    if (step) {
        L.POP = c.take(PE);  L.PB = c.take(PE);
        L.PBCOST = c.take(P);  L.STAG = c.take(P);  L.SS = c.take(P);  L.DIST = c.take(P);  L.TMP = c.take(2 * P);
        L.GB = c.take(align2(D));  L.SC = c.take(MBX_NSCALAR);  L.DG = c.take(MBX_NRLPSO_DIAG_SLOTS);
        L.PNI = c.template take<int>(align2((kNrK * NP + 1) / 2));  L.GNI = c.template take<int>(4);
        L.DM = cached ? c.take(align2((int64_t)NP * nr_stride(NP))) : nullptr;
    }
    return L;
}
__host__ __device__ inline int64_t nr_lds_doubles(int rows, int NP, int D, bool step, bool cached) { LdsSize c; nr_layout(c, rows, NP, D, step, cached); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ NrLds nr_carve(double* base, int rows, int NP, int D, bool step, bool cached)
{
    const int64_t NE = align2((int64_t)rows * D), ZS = eval_z_doubles(rows, D), DD = align2((int64_t)D * D), P = align2(NP);
    NrLds L{};
    double* p = base;
    L.X = p; p += NE;  L.T = p; p += eval_t_doubles(rows, D);  L.Z = p; p += ZS;  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);
    L.NC = p; p += align2(rows);  L.RED = p; p += 32;  L.COST = p; p += P;
    L.POP = L.X;
    if (step) {
        L.POP = p; p += align2((int64_t)NP * D);  L.PB = p; p += align2((int64_t)NP * D);
        L.PBCOST = p; p += P;  L.STAG = p; p += P;  L.SS = p; p += P;  L.DIST = p; p += P;  L.TMP = p; p += 2 * P;
        L.GB = p; p += align2(D);  L.SC = p; p += MBX_NSCALAR;  L.DG = p; p += MBX_NRLPSO_DIAG_SLOTS;
        L.PNI = (int*)p; p += align2((kNrK * NP + 1) / 2);  L.GNI = (int*)p; p += 4;
        L.DM = cached ? p : nullptr;
    }
    return L;
}

// ------------------------------------------------------------------------------------------------ SAHLPSO (mbx_sahlpso.hpp)
constexpr int kShNP = MBX_SAHL_NP;
static_assert(kShNP % 2 == 0, "an int array of kShNP entries is a whole number of doubles");

struct ShLds {
    double *XR, *T, *Z, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *X, *V, *PB, *FX, *PC0, *W, *PCR, *NFCR, *NSCR, *PLS, *NFLS, *NSLS, *CDFCR, *CDFLS, *MCAU;
    int *RANK, *SELF, *MI, *MCR, *MLS, *MSUC;
    uint32_t* KEY;
    __device__ __forceinline__ EvalLds eval(const double* x, double* f) const { return EvalLds{x, Z, T, M1T, M2T, DSH, V0, V1, V2, f}; }
};

// rows = evaluation rows of the launch: 40 for the reset (XR is the population), 1 for a generation (step = true: the resident arrays as well)
MBX_LDS_WALK ShLds sh_layout(C& c, int rows, int D, bool step)
{
    const int64_t I = kShNP / 2;
    ShLds L{};
    lds_eval_prefix(c, rows, D, L.XR, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(align2(rows));  L.RED = c.take(32);
    L.RANK = c.template take<int>(I);  L.SELF = c.template take<int>(I);  L.MI = c.template take<int>(I);  L.MCR = c.template take<int>(I);
    L.MLS = c.template take<int>(I);  L.MSUC = c.template take<int>(I);  L.KEY = c.template take<uint32_t>(I);
    if (step) {
        const int64_t PE = align2((int64_t)kShNP * D);
        L.X = c.take(PE);  L.V = c.take(PE);  L.PB = c.take(PE);
        L.FX = c.take(kShNP);  L.PC0 = c.take(kShNP);  L.W = c.take(kShNP);  L.MCAU = c.take(kShNP);
        L.PCR = c.take(16);  L.NFCR = c.take(16);  L.NSCR = c.take(16);  L.PLS = c.take(16);  L.NFLS = c.take(16);  L.NSLS = c.take(16);
        L.CDFCR = c.take(16);  L.CDFLS = c.take(16);
    }
    return L;
}
__host__ __device__ inline int64_t sh_lds_doubles(int rows, int D, bool step) { LdsSize c; sh_layout(c, rows, D, step); return align2(c.n); }
__device__ __forceinline__ ShLds sh_carve(double* base, int rows, int D, bool step) { LdsCarve c{base}; return sh_layout(c, rows, D, step); }

// ------------------------------------------------------------------------------------------------ LES (mbx_les.hpp)
constexpr int kLesNP = MBX_LES_NP, kLesNParam = MBX_LES_NPARAM;
static_assert(kLesNP % 2 == 0 && kLesNParam % 2 == 0, "a float array of kLesNP or kLesNParam entries is a whole number of doubles");

struct LesLds {
    double *XR, *T, *Z, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *ZN, *MU, *SIG, *PC, *PS;
    float *PRM, *Q, *K, *V, *A, *W, *AL;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{XR, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

MBX_LDS_WALK LesLds les_layout(C& c, int D)
{
    const int64_t DV = align2(D);
    LesLds L{};
    lds_eval_prefix(c, kLesNP, D, L.XR, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(kLesNP);  L.RED = c.take(32);
    L.ZN = c.take(align2((int64_t)kLesNP * D));  L.MU = c.take(DV);  L.SIG = c.take(DV);  L.PC = c.take(3 * DV);  L.PS = c.take(3 * DV);
    L.PRM = c.template take<float>(kLesNParam / 2);  L.Q = c.template take<float>(kLesNP * 4);  L.K = c.template take<float>(kLesNP * 4);
    L.V = c.template take<float>(kLesNP / 2);  L.A = c.template take<float>(kLesNP / 2);  L.W = c.template take<float>(kLesNP / 2);
    L.AL = c.template take<float>(DV);                           // 2 align2(D) floats
    return L;
}
__host__ __device__ inline int64_t les_lds_doubles(int D) { LdsSize c; les_layout(c, D); return align2(c.n); }
__device__ __forceinline__ LesLds les_carve(double* base, int D) { LdsCarve c{base}; return les_layout(c, D); }

// ------------------------------------------------------------------------------------------------ L2L (mbx_l2l.hpp)
struct L2lLds {
    double *XR, *T, *Z, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *ACT, *IN, *H, *C, *HO, *CURVE;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{XR, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

// one evaluation row; ACT: the 128 activated gates, HO: sigmoid(o) tanh(c'), CURVE: cost[::2]
MBX_LDS_WALK L2lLds l2l_layout(C& c, int D)
{
    L2lLds L{};
    lds_eval_prefix(c, 1, D, L.XR, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(2);  L.ACT = c.take(MBX_L2L_GATES);  L.IN = c.take(align2(D + 2));  L.H = c.take(align2(D));
    L.C = c.take(MBX_L2L_HID);  L.HO = c.take(MBX_L2L_HID);  L.CURVE = c.take(MBX_L2L_CURVE);
    return L;
}
__host__ __device__ inline int64_t l2l_lds_doubles(int D) { LdsSize c; l2l_layout(c, D); return align2(c.n); }
__device__ __forceinline__ L2lLds l2l_carve(double* base, int D) { LdsCarve c{base}; return l2l_layout(c, D); }

// ------------------------------------------------------------------------------------------------ SYMBOL (mbx_symbol.hpp)
struct SymLds {
    double *A, *Bf, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *PBC, *GB, *GW, *CB, *RED, *PB, *DX, *PCST, *CST;
    int *FLAG, *TOK, *PROG;
    uint8_t* IDX;
    // the evaluator's rows are the candidates (`cand`); the buffer of the positions they were moved from is its scratch Z
    __device__ __forceinline__ EvalLds eval(double* cand, double* scratch) const { return EvalLds{cand, scratch, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

// A | Bf: the two position buffers, x and the candidates by turns (each as long as the evaluator's scratch Z, whose part the other one plays during an
// evaluation); PB | DX: pbest_pos and delta_x where they fit (`resident`), else they stay in the state block: the move reads only its own element of
// them.  TOK / CST: the rule by slot; PCST / PROG: the same in post-order; IDX: the index rows of a sub-step, bytes.
MBX_LDS_WALK SymLds sym_layout(C& c, int NP, int D, bool resident)
{
    const int64_t P = align2(NP), NE = align2((int64_t)NP * D), DV = align2(D);
    SymLds L{};
    L.A = c.take(eval_z_doubles(NP, D));  L.Bf = c.take(eval_z_doubles(NP, D));  L.T = c.take(eval_t_doubles(NP, D));
    lds_eval_consts(c, D, true, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(P);  L.PBC = c.take(P);  L.GB = c.take(DV);  L.GW = c.take(DV);  L.CB = c.take(DV);  L.RED = c.take(16);
    L.PB = c.take(resident ? NE : 0);  L.DX = c.take(resident ? NE : 0);
    L.PCST = c.take(64);  L.CST = c.take(64);
    L.FLAG = c.template take<int>(align2((P + 1) / 2));  L.TOK = c.template take<int>(32);  L.PROG = c.template take<int>(32);
    L.IDX = c.template take<uint8_t>(align2(((int64_t)MBX_SYM_RANDX_MAX * NP + 7) / 8));
    return L;
}
__host__ __device__ inline int64_t sym_lds_doubles(int NP, int D, bool resident) { LdsSize c; sym_layout(c, NP, D, resident); return c.n; }
// pbest_pos and delta_x on chip wherever the whole set fits the 160 KB of a gfx950 workgroup NEXT TO the kernels' static LDS: the block votes of sym_check
// (__syncthreads_count / __syncthreads_or) take 256 B of it in k_symbol_step and k_symbol_run.  kSymStaticLdsMax is the room left for that; symbol_prepare
// holds every kernel's static size against it.  (The largest geometry, NP 128 / D 40, is 159040 B without the two arrays: it fits with the room to spare.)
constexpr int64_t kSymStaticLdsMax = 1024, kSymLdsLimit = 160 * 1024;
__host__ __device__ inline bool sym_resident(int NP, int D) { return sym_lds_doubles(NP, D, true) * 8 + kSymStaticLdsMax <= kSymLdsLimit; }
__device__ __forceinline__ SymLds sym_carve(double* base, int NP, int D, bool resident) { LdsCarve c{base}; return sym_layout(c, NP, D, resident); }

// ------------------------------------------------------------------------------------------------ QLPSO (mbx_qlpso.hpp)
struct QlLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *POP, *COST, *MEAN, *DIST, *SC;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

// rows = evaluation rows of the launch: NP for the reset (its X doubles as the population), 1 for a step
MBX_LDS_WALK QlLds ql_layout(C& c, int rows, int NP, int D)
{
    const int64_t P = align2(NP);
    QlLds L;
    lds_eval_prefix(c, rows, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.MEAN = c.take(align2(D));
    L.NC = c.take(align2(rows));  L.RED = c.take(16);  L.POP = c.take(align2((int64_t)NP * D));  L.COST = c.take(P);  L.DIST = c.take(P);
    L.SC = c.take(MBX_NSCALAR);
    return L;
}
__host__ __device__ inline int64_t ql_lds_doubles(int rows, int NP, int D) { LdsSize c; ql_layout(c, rows, NP, D); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ QlLds ql_carve(double* base, int rows, int NP, int D)
{
    const int64_t NE = align2((int64_t)rows * D), SC = eval_z_doubles(rows, D), DD = align2((int64_t)D * D), P = align2(NP);
    QlLds L;
    double* p = base;
    L.X = p; p += NE;  L.T = p; p += eval_t_doubles(rows, D);  L.Z = p; p += SC;  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);  L.MEAN = p; p += align2(D);
    L.NC = p; p += align2(rows);  L.RED = p; p += 16;  L.POP = p; p += align2((int64_t)NP * D);  L.COST = p; p += P;  L.DIST = p; p += P;
    L.SC = p;
    return L;
}

// ------------------------------------------------------------------------------------------------ RL-PSO (mbx_rlpso.hpp)
struct RpLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *GB, *XC, *SC;
    float* ACTV;            // policy activations: input [2D] | h1 [2 h1] | h2 [2 h2] | out [2]
    float* WTS;             // packed actor weights (mbx_rlpso_rollout only)
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

constexpr int kRpActDoubles = 192;       // room for 2D + 2 h1 + 2 h2 + 2 floats (checked on the host)

// `rows` = evaluation rows the launch needs: NP for the reset, 1 for a step (17 KB instead of 27 KB at D = 10: the step kernel is a
// chain of short latency-bound phases, so the number of resident workgroups per CU is what buys throughput).
// weight_floats: the packed actor the launch brings (0 without one); WTS runs to the end of what the launch was given, so the carve needs no count
MBX_LDS_WALK RpLds rp_layout(C& c, int rows, int D, int weight_floats)
{
    RpLds L;
    lds_eval_prefix(c, rows, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.GB = c.take(align2(D));  L.XC = c.take(align2(D));
    L.NC = c.take(align2(rows));  L.RED = c.take(16);  L.SC = c.take(MBX_NSCALAR);
    L.ACTV = c.template take<float>(kRpActDoubles);
    L.WTS = c.template take<float>(align2((weight_floats + 1) / 2));
    return L;
}
__host__ __device__ inline int64_t rp_lds_doubles(int rows, int D, int weight_floats) { LdsSize c; rp_layout(c, rows, D, weight_floats); return c.n; }
// written out by hand, as before the walks: through the walk this family's kernels measured slower than the parent's (docs/EXPERIMENTS.md "One walk per LDS layout");
// the size above is the walk's and tests/lds_sizes_main.hip holds these pointers to the walk's over its grid
__host__ __device__ __forceinline__ RpLds rp_carve(double* base, int rows, int D)
{
    const int64_t NE = align2((int64_t)rows * D), SC = eval_z_doubles(rows, D), DD = align2((int64_t)D * D), P = align2(rows);
    RpLds L;
    double* p = base;
    L.X = p; p += NE;  L.T = p; p += eval_t_doubles(rows, D);  L.Z = p; p += SC;  L.M1T = p; p += DD;  L.M2T = p; p += DD;
    L.DSH = p; p += align2(D);  L.V0 = p; p += align2(D);  L.V1 = p; p += align2(D);  L.V2 = p; p += align2(D);
    L.GB = p; p += align2(D);  L.XC = p; p += align2(D);
    L.NC = p; p += P;  L.RED = p; p += 16;  L.SC = p; p += MBX_NSCALAR;  L.ACTV = reinterpret_cast<float*>(p); p += kRpActDoubles;
    L.WTS = reinterpret_cast<float*>(p);
    return L;
}

// ------------------------------------------------------------------------------------------------ DE / PSO / CMA-ES (mbx_classic.hpp)
struct ClLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED, *POP, *COST, *GB, *SC, *C, *B, *VEC;
    int* ORD;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

// rows: evaluation rows of the launch; pop: 1 if the population is kept in LDS (DE sweeps); cma: 1 for the CMA-ES matrices
MBX_LDS_WALK ClLds cl_layout(C& c, int rows, int NP, int D, int pop, int cma)
{
    const int64_t DD = align2((int64_t)D * D), P = align2(NP);
    ClLds L;
    lds_eval_prefix(c, rows, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.GB = c.take(align2(D));
    L.NC = c.take(align2(rows));  L.RED = c.take(32);  L.SC = c.take(MBX_NSCALAR);  L.COST = c.take(P);
    L.ORD = c.template take<int>(align2((P + 1) / 2));
    L.POP = c.take(pop ? align2((int64_t)NP * D) : 0);
    // C | B and the Jacobi work matrix behind it | eight vectors and the weights: nothing stands behind the pointers unless cma
    L.C = c.take(cma ? DD : 0);  L.B = c.take(cma ? 2 * DD : 0);  L.VEC = c.take(cma ? 8 * align2(D) + P : 0);
    return L;
}
__host__ __device__ inline int64_t cl_lds_doubles(int rows, int NP, int D, int pop, int cma) { LdsSize c; cl_layout(c, rows, NP, D, pop, cma); return c.n; }
__device__ __forceinline__ ClLds cl_carve(double* base, int rows, int NP, int D, int pop, int cma) { LdsCarve c{base}; return cl_layout(c, rows, NP, D, pop, cma); }

// ------------------------------------------------------------------------------------------------ Random_search (mbx_rs.hpp)
struct RsLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *NC, *RED;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, NC}; }
};

MBX_LDS_WALK RsLds rs_layout(C& c, int NP, int D)
{
    RsLds L;
    lds_eval_prefix(c, NP, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.NC = c.take(align2(NP));  L.RED = c.take(16);
    return L;
}
__host__ __device__ inline int64_t rs_lds_doubles(int NP, int D) { LdsSize c; rs_layout(c, NP, D); return c.n; }
// the kernel carves inline, as before the walks (through the walk it measured slower than the parent's: docs/EXPERIMENTS.md "One walk per LDS layout")

// ------------------------------------------------------------------------------------------------ stand-alone evaluation (k_eval in mbx.hip)
// Random_search's layout without the reduction scratch: the costs F of `rows` rows end it
struct EvLds {
    double *X, *Z, *T, *M1T, *M2T, *DSH, *V0, *V1, *V2, *F;
    __device__ __forceinline__ EvalLds eval() const { return EvalLds{X, Z, T, M1T, M2T, DSH, V0, V1, V2, F}; }
};

MBX_LDS_WALK EvLds ev_layout(C& c, int rows, int D)
{
    EvLds L;
    lds_eval_prefix(c, rows, D, L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2);
    L.F = c.take(align2(rows));
    return L;
}
__host__ __device__ inline int64_t ev_lds_doubles(int rows, int D) { LdsSize c; ev_layout(c, rows, D); return c.n; }
// the kernel carves inline, as before the walks (through the walk it measured slower than the parent's: docs/EXPERIMENTS.md "One walk per LDS layout")

#undef MBX_LDS_WALK

}  // namespace mbx
