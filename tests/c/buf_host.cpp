// sfa::Buf (sigfish_amd/csrc/sfa_buf.hpp) on a counting malloc / free policy, built with -fsanitize=address,undefined
// (tests/test_c_host.py): growth rule, failure, moves, and that a scope of buffers leaves nothing behind.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "sfa_buf.hpp"

std::string &sfa::last_error_slot() {
    static std::string err;
    return err;
}

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                              \
        }                                                            \
    } while (0)

struct Counting {
    static constexpr const char *name = "testAlloc";
    static inline int allocs = 0, frees = 0, double_frees = 0;
    static inline bool fail_next = false;
    static inline std::set<void *> live;
    static inline std::vector<void *> freed;  // in order
    static void *alloc(size_t n) {
        if (fail_next) {
            fail_next = false;
            return nullptr;
        }
        void *p = malloc(n);
        ++allocs;
        live.insert(p);
        return p;
    }
    static void free(void *p) {
        if (!live.erase(p)) ++double_frees;
        ++frees;
        freed.push_back(p);
        ::free(p);
    }
};
using B = sfa::Buf<Counting>;

static_assert(!std::is_copy_constructible<B>::value && !std::is_copy_assignable<B>::value, "a buffer has one owner");
static_assert(std::is_nothrow_move_constructible<B>::value && std::is_nothrow_move_assignable<B>::value, "and can change it");

size_t grown(size_t bytes) { return bytes + bytes / 8 + 256; }

}  // namespace

int main() {
    {
        B b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(0) == SFA_OK && b.p == nullptr && Counting::allocs == 0);  // nothing asked for, nothing allocated
        CHECK(b.reserve(1000) == SFA_OK && b.p && b.cap == grown(1000));
        CHECK(Counting::allocs == 1 && Counting::frees == 0);
        static_cast<char *>(b.p)[b.cap - 1] = 1;  // the whole capacity is the buffer's (ASan)
        // below and at the capacity: no allocation, the pointer stays
        void *const p0 = b.p;
        for (size_t bytes : {size_t(1), size_t(1000), grown(1000)}) CHECK(b.reserve(bytes) == SFA_OK && b.p == p0 && b.cap == grown(1000));
        CHECK(Counting::allocs == 1 && Counting::frees == 0);
        // growth: the old block is freed, once, before the new one is allocated
        const size_t more = grown(1000) + 1;
        CHECK(b.reserve(more) == SFA_OK && b.cap == grown(more) && b.as<char>() != nullptr);
        CHECK(Counting::allocs == 2 && Counting::frees == 1 && Counting::freed.back() == p0 && Counting::live.size() == 1);
        // a failing allocator: the buffer is empty, the old block gone, the message names the call and the size asked for
        void *const p1 = b.p;
        Counting::fail_next = true;
        sfa::last_error_slot().clear();
        const size_t big = 1 << 20;
        CHECK(b.reserve(big) == SFA_ENOMEM && b.p == nullptr && b.cap == 0);
        CHECK(Counting::frees == 2 && Counting::freed.back() == p1 && Counting::live.empty());
        CHECK(sfa::last_error_slot() == "testAlloc(" + std::to_string(grown(big)) + " bytes) failed");
        // ... and it is usable again afterwards
        CHECK(b.reserve(16) == SFA_OK && b.cap == grown(16) && Counting::live.size() == 1);
    }
    CHECK(Counting::live.empty() && Counting::allocs == Counting::frees);  // the destructor freed the last block

    {   // moves: ownership travels, the source is empty, what the target held before is freed
        B a, c;
        CHECK(a.reserve(100) == SFA_OK && c.reserve(200) == SFA_OK);
        void *const pa = a.p, *const pc = c.p;
        const int frees0 = Counting::frees;
        B m(std::move(a));
        CHECK(m.p == pa && m.cap == grown(100) && a.p == nullptr && a.cap == 0 && Counting::frees == frees0);
        c = std::move(m);
        CHECK(c.p == pa && c.cap == grown(100) && m.p == nullptr && m.cap == 0);
        CHECK(Counting::frees == frees0 + 1 && Counting::freed.back() == pc && Counting::live.size() == 1);
        B &self = c;
        c = std::move(self);  // self-assignment keeps the block
        CHECK(c.p == pa && Counting::frees == frees0 + 1);
        CHECK(a.reserve(50) == SFA_OK && a.cap == grown(50));  // a moved-from buffer is an empty one
    }
    CHECK(Counting::live.empty() && Counting::allocs == Counting::frees);

    {   // a scope holding several buffers, some of them grown, one never used, one moved into a container
        struct Group {
            B x, y, z, unused;
        } g;
        std::vector<B> v;
        for (size_t bytes : {size_t(10), size_t(5000), size_t(100000)})
            CHECK(g.x.reserve(bytes) == SFA_OK && g.y.reserve(2 * bytes) == SFA_OK && g.z.reserve(7) == SFA_OK);
        v.push_back(std::move(g.z));
        v.emplace_back();
        CHECK(v.back().reserve(33) == SFA_OK);
        CHECK(Counting::live.size() == 4);
    }
    CHECK(Counting::live.empty() && Counting::allocs == Counting::frees && Counting::double_frees == 0);

    printf("%d allocations, %d frees, %d live, %d failures\n", Counting::allocs, Counting::frees, static_cast<int>(Counting::live.size()), failures);
    return failures ? 1 : 0;
}
