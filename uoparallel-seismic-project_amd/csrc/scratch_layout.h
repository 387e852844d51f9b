// scratch_layout.h - where the arrays of one call lie in one block of device memory, and the shift arithmetic of
// the int64 fixed-point sums.  Nothing of HIP here: the rules are plain host arithmetic, so that a stand-alone
// program can check them on the CPU (tests/host/scratch_layout_main.cpp, under the sanitizers).
#pragma once

#include <cstddef>
#include <cstring>
#include <utility>
#include <vector>

namespace ttsweep {

constexpr size_t SCRATCH_ALIGN = 256;

// add() declares the arrays of a call; place(base) sets their pointers, in the order of their declaration, into a
// block of at least size() bytes whose base is aligned to SCRATCH_ALIGN: each array starts on a multiple of
// SCRATCH_ALIGN and size() is the end of the last one.  The pointers handed to add() must outlive the layout.
class ScratchLayout {
    size_t bytes = 0;
    std::vector<std::pair<void *, size_t>> slots;      // where a pointer is kept, and its offset

public:
    template <typename T>
    void add(T *&ptr, size_t n)
    {
        const size_t at = (bytes + SCRATCH_ALIGN - 1) & ~(SCRATCH_ALIGN - 1);
        slots.push_back({&ptr, at});
        bytes = at + n * sizeof(T);
    }
    size_t size() const { return bytes; }
    void place(char *base) const
    {
        for (const auto &s : slots) {
            char *q = base + s.second;
            memcpy(s.first, &q, sizeof(q));
        }
    }
};

// the smallest k with 2^k >= n (0 for n <= 1): K of the shifts S = 61 - E - K of the fixed-point sums
inline int ceil_log2(long long n)
{
    int k = 0;
    while ((1LL << k) < n) k++;
    return k;
}

} // namespace ttsweep
