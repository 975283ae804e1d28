// lds_sizes_gleet_main.hip — prints, for every "NP D" pair on its command line, what the resident GLEET rollout's LDS walk (glr_layout, mbx_lds.hpp) and
// the generation kernel's (gl_layout) make of that geometry, one "name value" pair per line, byte offsets from the base of the dynamic LDS:
//   gl_<ptr> / glr_<ptr>   the evaluator prefix and the generation's own arrays under either walk
//   gl_doubles glr_doubles where the walks end (the sizes the host launches with)
//   t_begin z_end          the evaluator's scratch T | Z
//   kl vl kv_end pred      the actor's keys, values and block-sum slots
// Host code only: it launches nothing and runs on a machine without a GPU (tests/test_gleet_resident.py builds and runs it).
#include "mbx_lds.hpp"
#include <cstdio>
#include <cstdlib>

using namespace mbx;

static double* const kBase = (double*)0x100000000ull;
static long long off(const void* p) { return (long long)((const char*)p - (const char*)kBase); }

static void prefix(const char* who, const GlLds& L)
{
    const void* ptr[] = {L.X, L.T, L.Z, L.M1T, L.M2T, L.DSH, L.V0, L.V1, L.V2, L.GB, L.NC, L.K1, L.K2, L.RED, L.GF, L.IMPR};
    const char* name[] = {"X", "T", "Z", "M1T", "M2T", "DSH", "V0", "V1", "V2", "GB", "NC", "K1", "K2", "RED", "GF", "IMPR"};
    for (int i = 0; i < 16; ++i) std::printf("%s_%s %lld\n", who, name[i], off(ptr[i]));
}

int main(int argc, char** argv)
{
    for (int a = 1; a + 1 < argc; a += 2) {
        const int NP = std::atoi(argv[a]), D = std::atoi(argv[a + 1]);
        LdsCarve c1{kBase}, c2{kBase};
        const GlLds G = gl_layout(c1, NP, D);
        const GlrLds R = glr_layout(c2, NP, D);
        std::printf("geometry %d %d\n", NP, D);
        prefix("gl", G);
        prefix("glr", R.g);
        std::printf("gl_doubles %lld\nglr_doubles %lld\n", (long long)gl_lds_doubles(NP, D), (long long)glr_lds_doubles(NP, D));
        std::printf("glr_carve_end %lld\n", off(c2.p));
        std::printf("t_begin %lld\nz_end %lld\n", off(R.g.T), off(R.g.Z + eval_z_doubles(NP, D)));
        std::printf("kl %lld\nvl %lld\nkv_end %lld\npred %lld\n", off(R.KL), off(R.VL), off(R.VL + 16 * NP), off(R.PRED));
    }
    return 0;
}
