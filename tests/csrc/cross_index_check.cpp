// cross_index_check.cpp -- csrc/fleet_index.h's cross_pair_count and cross_pair on the host (tests/test_cross_cpu.py compiles this with the
// address and undefined-behaviour sanitizers and runs it as a program).  Usage: cross_index_check m_a m_b first count out
// Writes, for the `count` pairs from `first` on, (i, j) as two uint32 each to `out`, after one uint32 with cross_pair_count(m_a, m_b).
// The test compares them with Python's divmod; what is asserted here is what the kernel's staging relies on: the pair count fits 32 bits
// with a trip's 128 places on top, and i < m_a, j < m_b.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fleet_index.h"

int main(int argc, char **argv)
{
    static_assert(rp::kCrossMost == 32768, "the largest fleet of a cross query");
    static_assert((uint64_t)rp::kCrossMost * rp::kCrossMost + 128 <= UINT32_MAX, "a pair index plus a trip's places stays inside 32 bits");
    if (argc != 6) return 2;
    const unsigned m_a = (unsigned)strtoul(argv[1], nullptr, 10), m_b = (unsigned)strtoul(argv[2], nullptr, 10);
    const unsigned first = (unsigned)strtoul(argv[3], nullptr, 10), count = (unsigned)strtoul(argv[4], nullptr, 10);
    const unsigned pairs = rp::cross_pair_count(m_a, m_b);
    if ((uint64_t)pairs != (uint64_t)m_a * m_b || (uint64_t)first + count > pairs) return 3;
    std::vector<uint32_t> out(1 + 2 * (size_t)count);
    out[0] = pairs;
    for (unsigned r = 0; r < count; ++r) {
        unsigned i, j;
        rp::cross_pair(first + r, m_b, i, j);
        if (i >= m_a || j >= m_b) return 4;
        out[1 + 2 * (size_t)r] = i;
        out[2 + 2 * (size_t)r] = j;
    }
    FILE *f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size()) return 5;
    fclose(f);
    return 0;
}
