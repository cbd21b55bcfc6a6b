// The state behind numerics.h, reached through functions only: the process default, the thread's one-shot, and the setters of the C ABI.
#include "numerics.h"
#include <cstdlib>

namespace mcr {

static int g_default_variant = []() {                   // env MCR_LOCAL_PCT_VARIANT picks the start-up value (testing: whole suites on a variant)
    const char* e = getenv("MCR_LOCAL_PCT_VARIANT");
    const int v = e ? atoi(e) : 6;
    return (v == 1 || v == 5 || v == 6) ? v : 6;
}();
static thread_local int t_next_variant = 0;             // one-shot: consumed by the next VariantScope of this thread
VariantScope::VariantScope() : nm_{t_next_variant ? t_next_variant : g_default_variant} { t_next_variant = 0; }

}  // namespace mcr

using namespace mcr;

extern "C" {

int mcr_set_local_pct_variant(int v) {
    MCR_REQUIRE(v == 1 || v == 5 || v == 6 || MCR_VARIANT8_OK(v), "mcr_set_local_pct_variant: the process default must be 1, 5 or 6 (got %d; 7, the opt-in 16-bit matrix path, is per call only: mcr_call_variant)", v);
    g_default_variant = v;
    return 0;
}
int mcr_get_local_pct_variant(void) { return g_default_variant; }
int mcr_call_variant(int v) {
    MCR_REQUIRE(v == 0 || v == 1 || v == 5 || v == 6 || v == 7 || MCR_VARIANT8_OK(v),
                "mcr_call_variant: variant must be 0 (default), 1, 5, 6 or 7 (the opt-in 16-bit matrix path) (got %d)", v);
    t_next_variant = v;
    return 0;
}

}  // extern "C"
