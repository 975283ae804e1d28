// mbx_run_sahlpso.hip — SAHLPSO: the kernels (mbx_sahlpso.hpp) and their host code, a translation unit of their own like mbx_run_nrlpso.hip; mbx.hip
// sees the row kSahlpsoOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_sahlpso.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int sahlpso_check(const mbx_algo_cfg& c)
{
    // 40 particles shrinking to 4 (8 of them exploration particles), one lane per dimension in the move; the 40 initial evaluations are spent by mbx_reset
    if (c.np != MBX_SAHL_NP) return fail(MBX_E_ARG, "SAHLPSO runs np = %d (shrinking to 4), not %d", MBX_SAHL_NP, c.np);
    if (c.dim < 2 || c.dim > MBX_SAHL_DIM_MAX) return fail(MBX_E_ARG, "SAHLPSO runs dim in [2, %d], not %d", MBX_SAHL_DIM_MAX, c.dim);
    if (c.max_fes <= MBX_SAHL_NP) return fail(MBX_E_ARG, "SAHLPSO needs max_fes > %d (the initial evaluation), not %d", MBX_SAHL_NP, c.max_fes);
    return MBX_OK;
}

static AlgoGeom sahlpso_geom(const mbx_algo_cfg& c) { return MBX_GEOM(SAHL, std::max(sh_lds_doubles(MBX_SAHL_NP, c.dim, false), sh_lds_doubles(1, c.dim, true)), 1, 0); }
static int sahlpso_prepare(mbx_batch*, const AlgoGeom& g) { return allow_lds(lds_of(g), k_sahlpso_reset, k_sahlpso_generation); }
MBX_RESET_FN(sahlpso_reset) { MBX_LAUNCH(k_sahlpso_reset, kThreads, (size_t)sh_lds_doubles(MBX_SAHL_NP, b->cfg.dim, false) * sizeof(double), d_state_out); }
MBX_STEP_FN(sahlpso_step) { MBX_LAUNCH(k_sahlpso_generation, kThreads, (size_t)sh_lds_doubles(1, b->cfg.dim, true) * sizeof(double), MBX_OUT); return MBX_OK; }

MBX_EXPORT_ROW(kSahlpsoOps, MBX_ALGO_SAHLPSO, "SAHLPSO", false, false, sahlpso_check, sahlpso_geom, sahlpso_prepare, sahlpso_reset, sahlpso_step, nullptr);

}  // namespace mbx
