// text_cache_affine_flags_selftest.cpp — check_flags (csrc/fr_host_rules.cpp) and FR_TEXT_CACHE_AFFINE: the flag passes only
// where an entry point names it as allowed (the two _affine text entry points, csrc/fr_api_plan.hip), alone or beside the
// other text flags; FR_TEXT_CACHE beside it, or an unassigned bit, is refused there too.  One line per case,
//   <case> rc=<code> ok | err=<message>
// which tests/test_text_cache_affine_tables.py reads.  Links fr_host_rules.o and nothing else of the library.
#include "../csrc/fr_host_rules.hpp"
#include "selftest.hpp"

using namespace selftest;

int main()
{
    const uint32_t rgba = FR_TEXT_SRGB | FR_TEXT_BGRA | FR_TEXT_LOAD | FR_TEXT_OVER, A = FR_TEXT_CACHE_AFFINE;
    const struct { const char *name; uint32_t flags, also; } CASES[] = {
        {"raster", A, 0u}, {"upright", A, FR_TEXT_CACHE}, {"upright-rgba", A, rgba | FR_TEXT_CACHE}, {"affine", A, A}, {"affine-fill", A | FR_FILL_CONSISTENT, A},
        {"affine-rgba-all", A | FR_FILL_CONSISTENT | rgba, rgba | A}, {"affine-coverage-srgb", A | FR_TEXT_SRGB, A}, {"both-caches-affine", A | FR_TEXT_CACHE, rgba | A},
        {"both-caches-upright", A | FR_TEXT_CACHE, rgba | FR_TEXT_CACHE}, {"bit1", A | 2u, rgba | A}, {"bit4", A | 16u, rgba | A}, {"bit6", A | 64u, rgba | A},
        {"top", A | 0x80000000u, rgba | A},
    };
    for (const auto &c : CASES) {
        clear_error();
        const int rc = fr::check_flags(c.flags, c.also);
        require((rc == FR_OK) == ((c.flags & ~(FR_FILL_CONSISTENT | c.also)) == 0u), c.name, "check_flags disagrees with the allowed mask");
        printf("%s rc=%d %s%s\n", c.name, rc, rc ? "err=" : "ok", rc ? last_error() : "");
    }
    return exit_status();
}
