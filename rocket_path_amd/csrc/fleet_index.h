// fleet_index.h -- the pairs of a fleet (internal; trajectory.hip, and the host: it includes nothing and compiles as plain C++).  The
// m (m - 1) / 2 pairs (i, j), i < j, of m vehicles are numbered in lexicographic order -- (0, 1), (0, 2), ..., (0, m - 1), (1, 2), ... --
// which is torch.triu_indices(m, m, 1)'s.  Integers only: no square root whose rounding would have to be proved.
#pragma once

#if defined(__HIPCC__)
#define RP_FLEET_INLINE __host__ __device__ __forceinline__
#else
#define RP_FLEET_INLINE inline
#endif

namespace rp {

constexpr unsigned kFleetMost = 256;      // vehicles per scene: 32,640 pairs at the most

RP_FLEET_INLINE unsigned fleet_pair_count(unsigned m) { return m * (m - 1u) / 2u; }

// pair r < fleet_pair_count(m) of m >= 2 vehicles: row i holds m - 1 - i pairs; at most m - 1 subtractions
RP_FLEET_INLINE void fleet_pair(unsigned r, unsigned m, unsigned &i, unsigned &j)
{
    unsigned first = 0, row = m - 1u;
    while (first + 2u < m && r >= row) {      // (the last row is where the walk ends whatever r is)
        r -= row;
        --row;
        ++first;
    }
    i = first;
    j = first + 1u + r;
}

// The pairs across two fleets of m_a and m_b vehicles: every vehicle i of A against every vehicle j of B, row-major --
// pair r is (r / m_b, r % m_b), so n x pairs x k is n x m_a x m_b x k.  32,768 a side: 2^30 pairs, and a pair index plus a trip's 128 places
// stays inside 32 bits.
constexpr unsigned kCrossMost = 32768;

RP_FLEET_INLINE unsigned cross_pair_count(unsigned m_a, unsigned m_b) { return m_a * m_b; }

// pair r < cross_pair_count(m_a, m_b) of 1 <= m_a, m_b <= kCrossMost vehicles
RP_FLEET_INLINE void cross_pair(unsigned r, unsigned m_b, unsigned &i, unsigned &j)
{
    i = r / m_b;
    j = r - i * m_b;
}

}  // namespace rp
