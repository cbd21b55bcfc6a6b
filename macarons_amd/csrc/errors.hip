// Error plumbing + library identity for the C-ABI (include/macarons_hip.h).
#include "common.h"
#include <stdarg.h>
#include <stdio.h>

namespace mcr {
static thread_local char g_err[512] = "";
static thread_local bool g_refused = false;       // a launcher refused its call since the last check_hip() on this thread

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    g_refused = false;                            // the entry is already on an error path of its own
}

void refuse(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    g_refused = true;
}

int check_hip(hipError_t e, const char* what) {
    if (g_refused) {                              // nothing was launched for (part of) the call: the launcher's message stands
        g_refused = false;
        return 3;
    }
    if (e == hipSuccess) return 0;
    set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
    return 2;
}
}  // namespace mcr

extern "C" {
const char* mcr_last_error(void) { return mcr::g_err; }
int mcr_abi_version(void) { return 1; }
const char* mcr_target_arch(void) { return "gfx950"; }
}
