// Device scratch of one entry point or launcher, from the ctx arena (host only).  A piece's size is written once:
//     double *dwp = nullptr; int32_t *dsr = nullptr;
//     Scratch s(ctx);
//     s.want(&dwp, nwp);                       // a typed pointer variable and an element count
//     if (state_log) s.want(&dsl, nsl);        // an optional piece: not registered, its pointer stays what the caller set
//     if (int rc = s.commit()) return rc;      // adds the sizes up, reserves the arena for exactly that, writes every pointer
// The host-pointer twins register their copies with the piece: in() uploads `n` elements in upload(), out() downloads them in
// download() (a null host pointer is skipped), inout() does both; each in registration order, through uavac_h2d / uavac_d2h.
// Scratch does not nest: a live Scratch marks the ctx, and the commit of a second one on a marked ctx fails instead of rewinding
// the first one's pieces.  The Scratch that holds the mark may register more and commit again; that lays all its pieces out
// anew (the arena may have moved), so what they held is lost.
#pragma once

#include <cstring>

#include "uavac_internal.h"

static inline size_t uavac_arena_size(size_t bytes) { return ((bytes ? bytes : 8) + 255) & ~(size_t)255; }

class Scratch {
  public:
    explicit Scratch(uavac_ctx *ctx) : ctx_(ctx) {}
    ~Scratch() {
        if (marked_) ctx_->scratch_live = false;
    }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;

    template <class T> void want(T **p, size_t count) { add(p, count * sizeof(T), nullptr, nullptr); }
    template <class T> void in(T **p, const T *host, size_t count) { add(p, count * sizeof(T), host, nullptr); }
    template <class T> void out(T **p, T *host, size_t count) { add(p, count * sizeof(T), nullptr, host); }
    template <class T> void inout(T **p, T *host, size_t count) { add(p, count * sizeof(T), host, host); }

    int commit() {
        if (n_ > kSlots) return uavac_fail(ctx_, UAVAC_EINVAL, "internal: more scratch pieces than a Scratch holds");
        if (ctx_->scratch_live && !marked_) return uavac_fail(ctx_, UAVAC_EINVAL, "internal: nested device scratch");
        size_t total = 0;
        for (int i = 0; i < n_; ++i) total += uavac_arena_size(slot_[i].bytes);
        if (int rc = uavac_arena_reserve(ctx_, total)) return rc;
        ctx_->scratch_live = marked_ = true;
        char *p = ctx_->d_arena;
        for (int i = 0; i < n_; ++i) {
            std::memcpy(slot_[i].var, &p, sizeof p);          // (the variable is a T *: written as the pointer it is)
            slot_[i].dev = p;
            p += uavac_arena_size(slot_[i].bytes);
        }
        return UAVAC_OK;
    }
    int upload() {
        for (int i = 0; i < n_; ++i)
            if (slot_[i].src)
                if (int rc = uavac_h2d(ctx_, slot_[i].dev, slot_[i].src, slot_[i].bytes)) return rc;
        return UAVAC_OK;
    }
    int download() {
        for (int i = 0; i < n_; ++i)
            if (slot_[i].dst)
                if (int rc = uavac_d2h(ctx_, slot_[i].dst, slot_[i].dev, slot_[i].bytes)) return rc;
        return UAVAC_OK;
    }

  private:
    struct Slot {
        void *var, *dev;
        size_t bytes;
        const void *src;
        void *dst;
    };
    static constexpr int kSlots = 16;      // the largest users: uavac_launch_optimize_times, uavac_minsnap_obstacle_waypoints
    void add(void *var, size_t bytes, const void *src, void *dst) {
        if (n_ < kSlots) slot_[n_] = Slot{var, nullptr, bytes, src, dst};
        ++n_;                              // (past kSlots only counted: commit() refuses)
    }
    uavac_ctx *ctx_;
    Slot slot_[kSlots];
    int n_ = 0;
    bool marked_ = false;
};
