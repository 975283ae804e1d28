// lds_sizes_main.hip — prints the dynamic-LDS size (in doubles) of every kernel family over a grid of geometries, one "name(args) doubles" line each.
// Host code only: it launches nothing and runs on a machine without a GPU.  tests/test_lds_sizes.py builds it, runs it and compares the lines with
// tests/golden/lds_sizes.json, which was recorded from the tree as it stood BEFORE the layouts moved into mbx_lds.hpp.  There the size functions
// lived in the kernel headers (same names, same signatures), which is what MBX_LDS_SIZES_KERNEL_HEADERS includes instead; k_eval's size was a
// static function of mbx.hip, restated below for that build only.
#ifdef MBX_LDS_SIZES_KERNEL_HEADERS
#include "mbx_rlepso.hpp"
#include "mbx_lde.hpp"
#include "mbx_lde_run.hpp"
#include "mbx_ddqn.hpp"
#include "mbx_dedqn.hpp"
#include "mbx_gleet.hpp"
#include "mbx_glpso.hpp"
#include "mbx_jde21.hpp"
#include "mbx_madde.hpp"
#include "mbx_nlshade.hpp"
#include "mbx_rlhpsde.hpp"
#include "mbx_sdmspso.hpp"
#include "mbx_nrlpso.hpp"
#include "mbx_sahlpso.hpp"
#include "mbx_les.hpp"
#include "mbx_qlpso.hpp"
#include "mbx_rlpso.hpp"
#include "mbx_classic.hpp"
#include "mbx_rs.hpp"
namespace mbx {
inline int64_t ev_lds_doubles(int rows, int D)       // eval_lds_bytes of mbx.hip, in doubles
{
    const int64_t NE = align2((int64_t)rows * D), SC = align2(NE > 2 * kThreads ? NE : 2 * kThreads), DD = align2((int64_t)D * D);
    return NE + eval_t_doubles(rows, D) + SC + 2 * DD + 4 * align2(D) + align2(rows);
}
}  // namespace mbx
#else
#include "mbx_lds.hpp"
#endif
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace mbx;

static void put(const char* name, std::initializer_list<long long> args, long long doubles)
{
    std::printf("%s(", name);
    const char* sep = "";
    for (long long a : args) { std::printf("%s%lld", sep, a); sep = ","; }
    std::printf(") %lld\n", doubles);
}

// the families whose size depends on the evaluation rows alone
static void rows_only(int rows, int D)
{
    put("ev", {rows, D}, ev_lds_doubles(rows, D));
    for (int wf : {0, 2883, 4386}) put("rp", {rows, D, wf}, rp_lds_doubles(rows, D, wf));
}

// every family that takes a free (NP, D)
static void free_geometry(int NP, int D)
{
    rows_only(NP, D);
    for (int maps = 0; maps < 2; ++maps) {
        put("rl", {NP, D, maps}, rl_lds_doubles(NP, D, maps));
        put("lde", {NP, D, maps}, lde_lds_doubles(NP, D, maps));
    }
    put("rl_z", {NP, D}, rl_z_doubles(NP, D));
    for (int H : {33, 50})
        for (int two = 0; two < 2; ++two) put("lde_run", {NP, D, H, two}, lde_run_lds_doubles(NP, D, H, two));
    put("dd", {NP, D}, dd_lds_doubles(NP, D));
    put("gl", {NP, D}, gl_lds_doubles(NP, D));
    put("gp", {NP, D}, gp_lds_doubles(NP, D));
    put("sd", {NP, D}, sd_lds_doubles(NP, D));
    put("rs", {NP, D}, rs_lds_doubles(NP, D));
    for (int rows : {1, NP}) {
        put("dq", {rows, NP, D}, dq_lds_doubles(rows, NP, D));
        put("ql", {rows, NP, D}, ql_lds_doubles(rows, NP, D));
        for (int pop = 0; pop < 2; ++pop)
            for (int cma = 0; cma < 2; ++cma) put("cl", {rows, NP, D, pop, cma}, cl_lds_doubles(rows, NP, D, pop, cma));
        for (int step = 0; step < 2; ++step)
            for (int cached = 0; cached < 2; ++cached) put("nr", {rows, NP, D, step, cached}, nr_lds_doubles(rows, NP, D, step, cached));
    }
#ifndef MBX_LDS_SIZES_KERNEL_HEADERS                 // SYMBOL and L2L were born as walks: a tree without mbx_lds.hpp has neither
    for (int resident = 0; resident < 2; ++resident) put("sym", {NP, D, resident}, sym_lds_doubles(NP, D, resident));
#endif
}

static int g_bad = 0;

#ifndef MBX_LDS_SIZES_KERNEL_HEADERS
// Eight families keep a carve written out by hand beside their walk (mbx_lds.hpp says why): every pointer of it must be the walk's.  The structs hold pointers only.
alignas(16) static double g_base[2];
template <class L> static void same(const char* name, const L& walk, const L& hand)
{
    static_assert(sizeof(L) % sizeof(void*) == 0, "pointers only");
    if (std::memcmp(&walk, &hand, sizeof(L)) != 0) { std::fprintf(stderr, "%s: the hand-written carve is not the walk's\n", name); g_bad = 1; }
}
#define SAME(f, carve_args, ...) { LdsCarve c_{g_base}; same(#f, f##_layout(c_, __VA_ARGS__), f##_carve carve_args); }
static void carves(int NP, int D)
{
    if (md_lds_hand_doubles(NP, D) != md_lds_doubles(NP, D)) { std::fprintf(stderr, "md_lds_hand_doubles(%d, %d) is not where the walk ends\n", NP, D); g_bad = 1; }
    SAME(dd, (g_base, NP, D), NP, D)  SAME(sd, (g_base, NP, D), NP, D)  SAME(md, (g_base, NP, D), NP, D)
    if (NP > MBX_JDE21_SNP) SAME(jd, (g_base, NP, D), NP, D)
    for (int rows : {1, NP}) {
        SAME(dq, (g_base, rows, NP, D), rows, NP, D)  SAME(ql, (g_base, rows, NP, D), rows, NP, D)
        SAME(rp, (g_base, rows, D), rows, D, 0)
        for (int step = 0; step < 2; ++step)
            for (int cached = 0; cached < 2; ++cached) SAME(nr, (g_base, rows, NP, D, (bool)step, (bool)cached), rows, NP, D, (bool)step, (bool)cached)
    }
}
#else
static void carves(int, int) {}
#endif

// the sorted-DE kernels (MadDE, NL_SHADE_LBC, RL-HPSDE)
static void sorted_de(int NP, int D)
{
    carves(NP, D);
    put("md_work", {NP, D}, md_work_doubles(NP, D));
    put("md", {NP, D}, md_lds_doubles(NP, D));
    put("nl", {NP, D}, nl_lds_doubles(NP, D));
    put("hp", {NP, D}, hp_lds_doubles(NP, D));
}

#ifndef MBX_LDS_SIZES_KERNEL_HEADERS
// "offsets": the byte offset of every pointer the walk-carved families hand their kernels (a word that is no pointer into the area prints as =value), in the
// format of tests/golden/lds_offsets.txt, which was recorded from the hand-written carves these walks replaced (their text compiled for the host)
template <class L> static void show(const char* name, std::initializer_list<long long> args, const L& l, size_t words = sizeof(L) / 8)
{
    static double* const base = (double*)0x100000000ull;
    std::printf("%s(", name); for (long long a : args) std::printf("%lld,", a); std::printf(")");
    unsigned long long w[sizeof(L) / 8 + 1] = {}; std::memcpy(w, &l, sizeof(L));
    for (size_t i = 0; i < words; ++i) { if (w[i] >= (unsigned long long)base) std::printf(" %llu", w[i] - (unsigned long long)base); else std::printf(" =%llu", w[i] & 0xffffffffull); }
    std::printf("\n");
}
#define WALK(f, ...) [&] { LdsCarve c_{(double*)0x100000000ull}; return f##_layout(c_, __VA_ARGS__); }()
static int offsets()
{
    for (int D : {2, 10, 12, 33})
        for (int NP : {4, 17, 40, 51, 100, 129, 256}) {
            for (int m = 0; m < 2; ++m) {
                show("rl", {NP, D, m}, WALK(rl, NP, D, (bool)m), sizeof(RlLds) / 8 - 1);      // without zd (rl_z in the sizes) and its padding
                show("lde", {NP, D, m}, WALK(lde, NP, D, (bool)m)); show("lde_run", {NP, D, m}, WALK(lde_run, NP, D, 50, (bool)m));
            }
            show("gl", {NP, D}, WALK(gl, NP, D)); show("gp", {NP, D}, WALK(gp, NP, D));
            for (int rows : {1, NP})
                for (int pop = 0; pop < 2; ++pop) show("cl", {rows, NP, D, pop}, WALK(cl, rows, NP, D, pop, 1));
            if (NP == 40) {
                for (int rows : {1, 40}) for (int st = 0; st < 2; ++st) show("sh", {rows, D, st}, WALK(sh, rows, D, (bool)st));
                show("les", {D}, WALK(les, D));
            }
        }
    return 0;
}
#endif

int main(int argc, char** argv)
{
#ifndef MBX_LDS_SIZES_KERNEL_HEADERS
    if (argc > 1 && !std::strcmp(argv[1], "offsets")) return offsets();
#endif
    const int NPS[] = {4, 9, 16, 17, 50, 51, 52, 100, 128, 129, 255, 256};
    const int DS[] = {2, 7, 8, 9, 10, 12, 30, 33, 40};
    for (int D : DS) {
        for (int NP : NPS) { free_geometry(NP, D); sorted_de(NP, D); if (NP > MBX_JDE21_SNP) put("jd", {NP, D}, jd_lds_doubles(NP, D)); }
        rows_only(1, D);
        // the fixed populations
        put("les", {D}, les_lds_doubles(D));
#ifndef MBX_LDS_SIZES_KERNEL_HEADERS
        put("l2l", {D}, l2l_lds_doubles(D));
#endif
        for (int rows : {1, MBX_SAHL_NP})
            for (int step = 0; step < 2; ++step) put("sh", {rows, D, step}, sh_lds_doubles(rows, D, step));
        put("jd", {MBX_JDE21_NP, D}, jd_lds_doubles(MBX_JDE21_NP, D));
        put("sd", {MBX_SDMS_NP, D}, sd_lds_doubles(MBX_SDMS_NP, D));
    }
    free_geometry(30, 10);                            // the shipped QLPSO / RL-PSO swarm: ql(1,30,10) is checked by hand in the test
    for (int D : {2, 10, 40})
        for (int NP : {MBX_MADDE_NP(D), MBX_NLSHADE_NP(D), MBX_RLHPSDE_NP(D)}) sorted_de(NP, D);
    return g_bad;
}
