// Host-only: the side streams of the SconeOcc forwards and the ONE guard that forks work onto them and joins it back.
#pragma once
#include "common.h"
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

namespace mcr {

// The global feature (a chain of ~20 small launches on 2048 tokens, ~0.3 ms of mostly latency) depends on nothing the local
// path produces and is needed only by the first head layer: it runs on a side stream beside the kNN / local-transformer
// launches (fork / join by events, so a captured graph keeps the structure).  MCR_OCC_OVERLAP=0 puts it back on the caller's stream.
struct OccSide { hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
// One side stream + fork / join event pair per (device, CALLER stream): two host streams (or threads) running SconeOcc
// concurrently never share an event pair; creation is serialised.
// slot 0: the global transformer / the cloud build; slot 1: the x embedding queued with the early part (its own stream: on slot 0 the
// cloud build of the first search would queue up behind its GEMMs)
inline OccSide* occ_side(hipStream_t caller, int slot = 0) {
    static const bool on = []() { const char* e = getenv("MCR_OCC_OVERLAP"); return !(e && e[0] == '0'); }();
    if (!on) return nullptr;
    static std::mutex mu;
    static std::map<std::pair<std::pair<int, int>, hipStream_t>, OccSide> table;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    OccSide& x = table[std::make_pair(std::make_pair(dev, slot), caller)];
    if (!x.s) {
        if (hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess) {
            x.s = nullptr;
            return nullptr;
        }
    }
    return &x;
}

// One branch of work beside the caller's stream s.  The constructor forks: it records side's fork event on s and makes the side stream
// wait for it.  The branch's work goes to stream() -- s itself when there is no side stream (side NULL) or the fork failed; forked()
// tells.  record() marks the branch's end on the side stream, join() makes s wait for that mark (so: record() first); both say whether
// HIP accepted the call and do nothing (true) on an unforked branch.  The destructor does whatever of the two is still missing, so
// every way out of an entry joins, error returns included: a dangling fork would poison a capture and let side-stream work outlive
// the caller's workspace.  The guard therefore exists before anything is queued on the side stream.
class SideBranch {
    OccSide* side_;
    hipStream_t s_;
    bool recorded_ = false, joined_ = false;
public:
    SideBranch(hipStream_t s, OccSide* side) : side_(side), s_(s) {
        if (side_ && !(hipEventRecord(side_->fork, s) == hipSuccess && hipStreamWaitEvent(side_->s, side_->fork, 0) == hipSuccess)) side_ = nullptr;
    }
    SideBranch(const SideBranch&) = delete;
    ~SideBranch() {
        if (!side_ || joined_) return;
        if (!recorded_) (void)record();
        (void)join();
    }
    bool forked() const { return side_ != nullptr; }
    hipStream_t stream() const { return side_ ? side_->s : s_; }
    bool record() { return !side_ || (recorded_ = hipEventRecord(side_->join, side_->s) == hipSuccess); }
    bool join() {
        if (!side_ || joined_) return true;
        joined_ = true;
        return hipStreamWaitEvent(s_, side_->join, 0) == hipSuccess;
    }
};

}  // namespace mcr
