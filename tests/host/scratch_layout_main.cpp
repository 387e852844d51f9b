// scratch_layout_main.cpp - exercises the layout of a call's device arrays and the shift arithmetic of the fixed-point
// sums (csrc/scratch_layout.h) on the CPU, in a host buffer; built with -fsanitize=address,undefined by
// tests/test_scratch_layout_cpu.py.  Exit status 0: every check held.
#include "scratch_layout.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace ttsweep;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

struct alignas(16) Sixteen {
    char b[16];
};

// an array declared in the layout: where its pointer is kept, and its bytes
struct Declared {
    void **slot;
    size_t bytes;
};

int main()
{
    static_assert(sizeof(Sixteen) == 16, "element of 16 bytes");
    const size_t lengths[5] = {0, 1, 63, 64, 65};
    // every length with every element size, in one layout; then each length first and each length last
    for (int rot = 0; rot < 5; rot++) {
        ScratchLayout lay;
        CHECK(lay.size() == 0);
        // (the vectors are sized first: the layout keeps the addresses of their elements)
        std::vector<char *> p1(5);
        std::vector<int32_t *> p4(5);
        std::vector<double *> p8(5);
        std::vector<Sixteen *> p16(5);
        std::vector<Declared> all;
        for (int i = 0; i < 5; i++) {
            const size_t n = lengths[(i + rot) % 5];
            lay.add(p1[i], n);
            all.push_back({reinterpret_cast<void **>(&p1[i]), n * 1});
            lay.add(p4[i], n);
            all.push_back({reinterpret_cast<void **>(&p4[i]), n * 4});
            lay.add(p8[i], n);
            all.push_back({reinterpret_cast<void **>(&p8[i]), n * 8});
            lay.add(p16[i], n);
            all.push_back({reinterpret_cast<void **>(&p16[i]), n * 16});
        }
        char *base = static_cast<char *>(aligned_alloc(SCRATCH_ALIGN, (lay.size() + SCRATCH_ALIGN - 1) / SCRATCH_ALIGN
                                                                           * SCRATCH_ALIGN));
        CHECK(base != nullptr);
        lay.place(base);
        const char *prev_end = base;
        for (const Declared &d : all) {
            const char *at = static_cast<const char *>(*d.slot);
            CHECK(reinterpret_cast<uintptr_t>(at) % SCRATCH_ALIGN == 0);      // aligned
            CHECK(at >= prev_end);                                            // declaration order, no overlap
            CHECK(at - prev_end < (ptrdiff_t)SCRATCH_ALIGN);                  // and no more than the padding between
            prev_end = at + d.bytes;
        }
        CHECK(prev_end == base + lay.size());           // the reported size is the end of the last array
        // every byte of every array can be written (the sanitizer watches the block's end)
        for (const Declared &d : all)
            for (size_t i = 0; i < d.bytes; i++) static_cast<char *>(*d.slot)[i] = (char)i;
        free(base);
    }
    // a layout placed a second time, elsewhere: the pointers follow
    {
        ScratchLayout lay;
        int32_t *a = nullptr;
        double *b = nullptr;
        lay.add(a, 3);
        lay.add(b, 2);
        CHECK(lay.size() == SCRATCH_ALIGN + 2 * sizeof(double));
        char *one = static_cast<char *>(aligned_alloc(SCRATCH_ALIGN, 2 * SCRATCH_ALIGN));
        char *two = static_cast<char *>(aligned_alloc(SCRATCH_ALIGN, 2 * SCRATCH_ALIGN));
        lay.place(one);
        CHECK((char *)a == one && (char *)b == one + SCRATCH_ALIGN);
        lay.place(two);
        CHECK((char *)a == two && (char *)b == two + SCRATCH_ALIGN);
        free(one);
        free(two);
    }
    // ---- ceil_log2: the smallest k with 2^k >= n
    CHECK(ceil_log2(1) == 0);
    CHECK(ceil_log2(2) == 1);
    CHECK(ceil_log2(3) == 2);
    CHECK(ceil_log2(1LL << 31) == 31);
    CHECK(ceil_log2((1LL << 31) + 1) == 32);
    CHECK(ceil_log2(0) == 0);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("scratch layout ok\n");
    return failures ? 1 : 0;
}
