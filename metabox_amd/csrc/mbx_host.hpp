// mbx_host.hpp — the host side every translation unit of libmbx.so shares: the handles behind include/mbx.h, the per-algorithm descriptor AlgoOps
// and the helpers an algorithm's block is written with.  Host code only: no kernel, nothing a kernel reads.  mbx.hip holds the single definitions
// of fail, max_lds_bytes and set_param_sets; an algorithm whose kernels live in a unit of their own (mbx_run_dedqn.hip ...) exports one row.
#ifndef MBX_HOST_HPP
#define MBX_HOST_HPP
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams

namespace mbx {
struct AlgoOps;
// parameter sets handed over per batch (LES: float32 [n_sets][246]; L2L: float64 [n_sets][MBX_L2L_NPARAM(dim)]) and the set of every instance; copies
struct ParamSets { void* d_params = nullptr; int32_t* d_set = nullptr; int n_sets = 0; };
}  // namespace mbx

// ------------------------------------------------------------------------------------------------ handles
struct mbx_suite {
    int n = 0, dim = 0;
    double* d_pool = nullptr;
    mbx::DevProblem* d_problems = nullptr;
    std::vector<mbx::DevProblem> h_problems;       // device pointers inside
    std::vector<double> optimum;
};

struct mbx_batch {
    mbx_suite* suite = nullptr;
    mbx_algo_cfg cfg{};
    const mbx::AlgoOps* ops = nullptr;     // the row of kAlgoOps for cfg.algo
    int B = 0;
    int32_t* d_problem_idx = nullptr;
    std::vector<int32_t> h_problem_idx;    // host copy (mbx_debug_write_state validates an injected block against its problem's box)
    uint64_t* d_seeds = nullptr;
    double* d_state = nullptr;
    int32_t* d_order = nullptr;
    double* d_pci = nullptr;               // RLEPSO: learning-probability curve [np]; DEDQN: correctly rounded log(n / np), n = 0 .. np
    unsigned long long* d_clk = nullptr;   // mbx_debug_clock_slots: the caller's slot block for the NEXT resident RLEPSO launches (not owned)
    double* d_scratch = nullptr; // [B] per-generation rewards of mbx_rlepso_rollout's host-loop route (RLEPSO batches; allocated by mbx_batch_create)
    float* d_lstm_pack = nullptr;          // k-blocked copy of the PolicyNet weights for k_lde_run (k_lde_repack at every mbx_lde_rollout call)
    bool fdr_fast = false;                 // RLEPSO, MBX_F_FDR_FAST honoured: the kernels without the near-tie flag / second pass of the FDR scan (include/mbx.h); cfg.flags holds
                                           // the EFFECTIVE flags (environment overrides OR-ed in, MBX_F_FDR_FAST cleared where no fast instantiation exists)
    bool lde_run_kinds_ok = false;         // LDE: every problem of the batch has an objective kind the LEAN instantiations of k_lde_run build (one tile array: lde_run_kind_ok(.., two = false))
    bool lde_run_kinds_two = false;        // ... a kind the instantiations with the second tile array build (F1-F24)
    bool nrlpso_cached = false;            // NRLPSO: the step kernels keep the NP x NP distance matrix in LDS (MBX_F_NRLPSO_RECOMPUTE clear and the matrix fits)
    mbx::ParamSets sets;                   // LES, L2L, GLEET: mbx_les_set_params / mbx_l2l_set_params / mbx_gleet_set_params
    float* d_les_ts = nullptr;             // LES: [les_horizon + 1][13] float32 timestamp embedding tanh(t / timestamp - 1), one row per generation counter
    int les_horizon = 0;
    float gleet_min_sigma = 0.f, gleet_max_sigma = 0.f;   // GLEET: the actor's sigma range, with the weight sets in `sets` (mbx_gleet_set_params)
    bool rollout_per_generation = false;   // MBX_F_ROLLOUT_PER_GENERATION: the mbx_*_rollout entry points take the host-loop route
    int64_t state_stride = 0;
    const double* d_tape = nullptr;
    size_t lds_bytes = 0;
    int64_t sc_off = 0;          // offset of the scalar block inside an instance's state
    int64_t tape_stride = 0;
    int state_dim = 0, action_dim = 0;
    int threads = mbx::kThreads; // workgroup size of the RLEPSO generation kernels (512 for LDS-bound geometries)
    // compile-time-geometry instantiation of the generation / rollout kernels (0 = geometry read from the batch):
    //   1 = RLEPSO NP 100 / D 10 / 5 groups (BASELINE configs 1-2)      2 = RLEPSO NP 128 / D 40 / 5 groups (config 5)      7 = RLEPSO NP 100 / D 30 (bbob --dim 30)
    //   8 / 10 = RLEPSO NP 100 at D 12 (protein docking) / D 40 (bbob --dim 40): resident kernel only, mbx_step stays on the run-time-geometry kernel
    //   3 / 6 = LDE NP 50 / NP 100 at D 30 (config 3)      9 = LDE NP 50 / D 10 (resident kernel only)      4 = DE-DDQN NP 100 / D 12 (config 4)      5 = GLEET NP 100 / D 10
    int fixed_geometry = 0;
};

namespace mbx {

// per-algorithm geometry
struct AlgoGeom { int64_t state_doubles, sc_off, tape_stride, lds_doubles; int state_dim, action_dim; };

// Everything the host code knows about one algorithm id: one block per algorithm and the table kAlgoOps in mbx.hip
struct AlgoOps {
    int id; const char* name;
    bool takes_actions;      // mbx_step refuses a null d_actions
    bool needs_state_out;    // mbx_reset / mbx_step refuse a null d_state_out: the kernels write the features without asking
    int (*check)(const mbx_algo_cfg&);                  // the algorithm's own limits; null = the common np in [4, kThreads]
    AlgoGeom (*geom)(const mbx_algo_cfg&);
    int (*prepare)(mbx_batch*, const AlgoGeom&);        // once per batch, at the end of mbx_batch_create
    void (*reset)(mbx_batch*, hipStream_t, double* d_state_out);
    int (*step)(mbx_batch*, hipStream_t, const void* d_actions, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
    void (*launch_info)(const mbx_batch*, int32_t out[4]);   // where the step kernel's figures differ from the batch's; null = they do not
    void (*bind)(mbx_batch*);                                // what the batch remembers about its problems, on create and on every rebind; null = nothing
};

// the rows defined beside their kernels (mbx_run_*.hip); mbx.hip's own rows are static there
extern const AlgoOps kDedqnOps, kNrlpsoOps, kSahlpsoOps, kLesOps, kL2lOps, kSymbolOps, kRlhpsdeOps, kNlshadeOps;
// A row is host data, but the device pass would emit an exported const with a constant initializer as well (the compiler makes such variables readable from
// kernels), host function pointers and all, and fail to link: that pass sees a file-local row, which it drops (and which keeps the block's functions used).
#ifdef __HIP_DEVICE_COMPILE__
#define MBX_EXPORT_ROW(name, ...) [[maybe_unused]] static const AlgoOps name##_device_pass = {__VA_ARGS__}
#else
#define MBX_EXPORT_ROW(name, ...) const AlgoOps name = {__VA_ARGS__}
#endif

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));      // leaves the text for mbx_last_error, returns code
int max_lds_bytes();
// mbx_les_set_params / mbx_l2l_set_params after their own argument checks: validates d_set_of_instance (may be null) against n_sets, replaces b->sets by copies
int set_param_sets(mbx_batch* b, const char* who, const void* d_params, size_t bytes_per_set, int n_sets, const int32_t* d_set_of_instance);

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail(MBX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

static inline int check_np(const mbx_algo_cfg& c) { return c.np < 4 || c.np > kThreads ? fail(MBX_E_ARG, "np %d outside [4, %d]", c.np, kThreads) : MBX_OK; }
static inline int check_dim(const mbx_algo_cfg& c) { return c.dim < 2 || c.dim > 64 ? fail(MBX_E_ARG, "dim %d outside [2, 64]", c.dim) : MBX_OK; }

static inline BatchParams make_params(const mbx_batch* b)
{
    BatchParams p;
    p.problems = b->suite->d_problems; p.problem_idx = b->d_problem_idx; p.seeds = b->d_seeds;
    p.state = b->d_state; p.state_stride = b->state_stride;
    p.tape = b->d_tape; p.tape_stride = b->tape_stride; p.order = b->d_order; p.pci = b->d_pci;
    p.NP = b->cfg.np; p.D = b->cfg.dim; p.max_fes = b->cfg.max_fes; p.log_interval = b->cfg.log_interval;
    p.n_logpoint = b->cfg.n_logpoint; p.early_stop = b->cfg.early_stop; p.n_group = b->cfg.n_group; p.B = b->B;
    p.sc_off = b->sc_off;
    p.clk = b->d_clk;
    return p;
}

// An algorithm's block: its limits (check), geometry (geom), per-batch setup (prepare: workgroup size / compile-time geometry, tables, and the
// kernels' dynamic-LDS limits), the reset launch and the one-step launch, then its row.  Templates are instantiated in the order a file first names
// them: keep the lists' order.
template <class... K>
static int allow_lds(size_t lds, K... kernels)
{
    for (const void* k : {(const void*)kernels...}) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MBX_OK;
}

static inline size_t lds_of(const AlgoGeom& g) { return (size_t)g.lds_doubles * sizeof(double); }
static inline bool generic_geometry(const mbx_batch* b) { return (b->cfg.flags & MBX_F_GENERIC_GEOMETRY) != 0; }   // keeps the run-time-geometry kernels (the tests compare the two instantiations bit for bit)

#define MBX_GEOM(P, lds, sdim, adim) \
    AlgoGeom{MBX_##P##_STATE_DOUBLES(c.np, c.dim, c.n_logpoint), MBX_##P##_ST_SCALARS(c.np, c.dim), MBX_##P##_TAPE_STRIDE(c.np, c.dim), (lds), (sdim), (adim)}
#define MBX_RESET_FN(name) static void name(mbx_batch* b, hipStream_t stream, double* d_state_out)
#define MBX_STEP_FN(name) static int name(mbx_batch* b, hipStream_t stream, const void* d_actions, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
#define MBX_OUT d_state_out, d_reward_out, d_done_out
// one workgroup per instance; a template-id with commas goes in parentheses
#define MBX_LAUNCH(kernel, threads, lds, ...) hipLaunchKernelGGL(kernel, dim3(b->B), dim3(threads), (lds), stream, make_params(b), __VA_ARGS__)

}  // namespace mbx
#endif  // MBX_HOST_HPP
