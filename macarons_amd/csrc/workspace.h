// Host-only: the caller's workspace.  ONE bump allocator with the one rounding rule, for every entry that takes (workspace, workspace_bytes):
// the network entries (through net_layout.h) and the depth module.  An entry describes its scratch as a struct of pointers with one carve
// function next to the code that uses it; its *_workspace_bytes runs that same function on a measuring arena, so the stated size and the
// layout cannot drift apart.
#pragma once
#include "common.h"

namespace mcr {

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Bump allocator over the caller's workspace (256-B aligned blocks).  Without a base it only measures: the carve functions run
// on it unchanged, hand out NULLs, and `off` is what they need.  ok(): nothing carved so far lies beyond the capacity.
struct Arena {
    char* base = nullptr; size_t cap = ~(size_t)0, off = 0;            // (as constructed by default: a measuring arena)
    void* bytes(size_t n) {
        char* p = base ? base + off : nullptr;
        off += align256(n);
        return p;
    }
    float* f(size_t n_floats) { return reinterpret_cast<float*>(bytes(n_floats * sizeof(float))); }
    bool ok() const { return off <= cap; }
    // what is left behind the carved part, as an arena of its own (a region alternatives reuse: each carves a copy of it)
    Arena rest() const { return Arena{base ? base + off : nullptr, off <= cap ? cap - off : 0}; }
};
// bytes `carve(arena, args...)` consumes
template <class Carve, class... A>
inline size_t measure(Carve carve, A... args) {
    Arena a;
    carve(a, args...);
    return a.off;
}

// The check of an entry whose *_workspace_bytes is exact (`need`): present, large enough, aligned for the 16-byte accesses.
inline int check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    MCR_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
    MCR_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    return 0;
}
// ... and of the networks' backward entries (their *_workspace_bytes includes a slack; their messages are matched by the tests as they are)
inline int check_bwd_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    MCR_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small", who);
    MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    return 0;
}

}  // namespace mcr
