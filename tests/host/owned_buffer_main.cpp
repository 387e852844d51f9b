// owned_buffer_main.cpp - exercises the owner of a block of device or pinned memory (csrc/owned_buffer.h) on the
// CPU, over a policy that sits on malloc / free, counts, records and fails on request; built with
// -fsanitize=address,undefined by tests/test_owned_buffer_cpu.py.  Exit status 0: every check held.
#include "owned_buffer.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

using namespace ttsweep;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int ERR_ALLOC = 2, ERR_RELEASE = 17;      // (what a runtime might return: handed on unchanged)

// malloc / free with a ledger.  A release that is told to fail keeps the block (the runtime refused it): the ledger
// frees such blocks itself at the end, so that the sanitizer's leak check judges the class and not the policy.
struct TestMem {
    static std::vector<void *> live, released, refused;
    static std::vector<size_t> sizes;               // bytes of every allocation that was asked for, in order
    static int fail_alloc, fail_release;            // fail the k-th call from now (1: the next one; 0: none)

    static int alloc(void **p, size_t bytes)
    {
        sizes.push_back(bytes);
        if (fail_alloc && --fail_alloc == 0) return ERR_ALLOC;
        *p = malloc(bytes);
        live.push_back(*p);
        return 0;
    }
    static int release(void *p)
    {
        CHECK(p != nullptr);
        CHECK(std::count(released.begin(), released.end(), p) == 0);   // never twice
        const auto at = std::find(live.begin(), live.end(), p);
        CHECK(at != live.end());                                        // and nothing that is not held
        if (at != live.end()) live.erase(at);
        released.push_back(p);
        if (fail_release && --fail_release == 0) {
            refused.push_back(p);
            return ERR_RELEASE;
        }
        free(p);
        return 0;
    }
    // (addresses come round again once freed: each scenario starts with an empty record)
    static void forget() { released.clear(); sizes.clear(); }
};
std::vector<void *> TestMem::live, TestMem::released, TestMem::refused;
std::vector<size_t> TestMem::sizes;
int TestMem::fail_alloc = 0, TestMem::fail_release = 0;

struct Twelve {
    int a[3];
};
template <class T> using Buf = OwnedBuffer<T, TestMem>;

static_assert(!std::is_copy_constructible<Buf<int>>::value, "a buffer has one owner");
static_assert(!std::is_copy_assignable<Buf<int>>::value, "a buffer has one owner");
static_assert(std::is_nothrow_move_constructible<Buf<int>>::value, "ownership moves");
static_assert(std::is_nothrow_move_assignable<Buf<int>>::value, "ownership moves");

template <class T>
static bool empty(const Buf<T> &b) { return b.get() == nullptr && b.count() == 0; }

int main()
{
    {   // alloc over a held buffer: one release, then exactly n * sizeof(T) bytes
        TestMem::forget();
        Buf<Twelve> b;
        CHECK(empty(b));
        CHECK(b.alloc(5) == 0);
        CHECK(b.get() != nullptr && b.count() == 5 && static_cast<Twelve *>(b) == b.get());
        CHECK(TestMem::sizes.size() == 1 && TestMem::sizes[0] == 5 * sizeof(Twelve) && TestMem::released.empty());
        for (size_t i = 0; i < b.count(); i++) b[i].a[2] = (int)i;      // (the sanitizer watches the block's end)
        Twelve *const first = b.get();
        CHECK(b.alloc(3) == 0);
        CHECK(b.count() == 3);
        CHECK(TestMem::released.size() == 1 && TestMem::released[0] == first);
        CHECK(TestMem::sizes.size() == 2 && TestMem::sizes[1] == 3 * sizeof(Twelve));
        CHECK(TestMem::live.size() == 1 && TestMem::live[0] == b.get());
        // reserve within the count: nothing allocated, nothing released, the pointer kept
        Twelve *const second = b.get();
        CHECK(b.reserve(3) == 0 && b.reserve(1) == 0 && b.reserve(0) == 0);
        CHECK(b.get() == second && b.count() == 3 && TestMem::sizes.size() == 2 && TestMem::released.size() == 1);
        // reserve beyond it: as alloc
        CHECK(b.reserve(4) == 0);
        CHECK(b.count() == 4 && TestMem::sizes.size() == 3 && TestMem::sizes[2] == 4 * sizeof(Twelve));
        CHECK(TestMem::released.size() == 2 && TestMem::released[1] == second);
        // alloc(0) and reset leave it empty
        CHECK(b.alloc(0) == 0);
        CHECK(empty(b) && TestMem::released.size() == 3 && TestMem::sizes.size() == 3 && TestMem::live.empty());
        CHECK(b.reset() == 0 && empty(b) && TestMem::released.size() == 3);
        CHECK(b.alloc(2) == 0 && b.reset() == 0);
        CHECK(empty(b) && TestMem::released.size() == 4 && TestMem::live.empty());
        CHECK(b.reserve(0) == 0 && empty(b) && TestMem::sizes.size() == 4);
    }
    CHECK(TestMem::live.empty());
    {   // a failed allocation: empty, the code handed on, and the buffer can be used again
        TestMem::forget();
        Buf<double> b;
        CHECK(b.alloc(4) == 0);
        TestMem::fail_alloc = 1;
        CHECK(b.alloc(8) == ERR_ALLOC);
        CHECK(empty(b) && TestMem::released.size() == 1 && TestMem::live.empty());
        TestMem::fail_alloc = 1;
        CHECK(b.reserve(8) == ERR_ALLOC && empty(b));
        CHECK(b.alloc(8) == 0 && b.count() == 8 && TestMem::sizes.back() == 8 * sizeof(double));
        b[7] = 1.0;
    }
    CHECK(TestMem::live.empty());
    {   // a failed release: empty, the code handed on, and the pointer never offered again - not by a later alloc,
        // not by the destructor
        TestMem::forget();
        {
            Buf<int> b;
            CHECK(b.alloc(4) == 0);
            int *const held = b.get();
            TestMem::fail_release = 1;
            CHECK(b.alloc(6) == ERR_RELEASE);
            CHECK(empty(b) && TestMem::sizes.size() == 1);       // (nothing was allocated after the refusal)
            CHECK(TestMem::released.size() == 1 && TestMem::released[0] == held);
            CHECK(b.alloc(6) == 0 && b.count() == 6);
            CHECK(TestMem::released.size() == 1);
            TestMem::fail_release = 1;
            CHECK(b.reset() == ERR_RELEASE && empty(b) && TestMem::released.size() == 2);
            CHECK(b.reset() == 0 && TestMem::released.size() == 2);
            CHECK(b.alloc(2) == 0);
            TestMem::fail_release = 1;
            CHECK(b.reserve(3) == ERR_RELEASE && empty(b) && TestMem::released.size() == 3);
        }
        CHECK(TestMem::released.size() == 3);       // (the destructor found nothing to release)
        {
            Buf<int> b;
            CHECK(b.alloc(1) == 0);
            TestMem::fail_release = 1;              // the destructor's own release fails: ignored
        }
        CHECK(TestMem::released.size() == 4 && TestMem::fail_release == 0);
    }
    CHECK(TestMem::live.empty());
    {   // moves hand the block on
        TestMem::forget();
        Buf<int> a;
        CHECK(a.alloc(4) == 0);
        int *const pa = a.get();
        Buf<int> b(std::move(a));
        CHECK(empty(a) && b.get() == pa && b.count() == 4 && TestMem::released.empty());
        Buf<int> c;
        CHECK(c.alloc(2) == 0);
        int *const pc = c.get();
        c = std::move(b);
        CHECK(empty(b) && c.get() == pa && c.count() == 4);
        CHECK(TestMem::released.size() == 1 && TestMem::released[0] == pc);     // the target's old block, once
        Buf<int> &self = c;
        c = std::move(self);
        CHECK(c.get() == pa && c.count() == 4 && TestMem::released.size() == 1);
        std::vector<Buf<int>> many(3);              // (buffers in a container: growing it moves them)
        CHECK(many[1].alloc(7) == 0);
        many.resize(40);
        CHECK(many[1].count() == 7 && TestMem::released.size() == 1);
    }
    CHECK(TestMem::released.size() == 3);           // c and many[1]; a and b had nothing left
    CHECK(TestMem::live.empty());                   // every block was released, none twice (TestMem::release)
    for (void *p : TestMem::refused) free(p);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("owned buffer ok\n");
    return failures ? 1 : 0;
}
