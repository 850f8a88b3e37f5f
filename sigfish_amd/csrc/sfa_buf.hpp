// sfa_buf.hpp -- the one buffer type of the context (sfa_ctx.hpp): grows, never shrinks, frees itself.  Batches reuse it, so
// nothing is allocated inside a steady-state call.  No HIP here: the allocator pair is the policy `Mem` { alloc(bytes) -> pointer
// or nullptr, free(pointer), name (of the allocating call, for the message) }, which lets tests/c/buf_host.cpp run the type on
// malloc / free under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>
#include <utility>

#include "../../include/sigfish_amd.h"

namespace sfa {
std::string &last_error_slot();  // this thread's sfa_last_error() text (sfa_context.hip)

template <class Mem>
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            drop();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~Buf() { drop(); }
    // at least `bytes`; a buffer that grows loses its contents (the old block is freed before the new one is asked for, so the
    // peak is one block) and gets an eighth of headroom
    int reserve(size_t bytes) {
        if (bytes <= cap) return SFA_OK;
        drop();
        const size_t want = bytes + bytes / 8 + 256;
        if (!(p = Mem::alloc(want))) {
            char msg[96];
            snprintf(msg, sizeof msg, "%s(%zu bytes) failed", Mem::name, want);
            last_error_slot() = msg;
            return SFA_ENOMEM;
        }
        cap = want;
        return SFA_OK;
    }
    template <typename T>
    T *as() const {
        return static_cast<T *>(p);
    }

  private:
    void drop() {
        if (p) Mem::free(p);
        p = nullptr;
        cap = 0;
    }
};
}  // namespace sfa
