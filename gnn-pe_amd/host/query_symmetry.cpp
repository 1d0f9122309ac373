// query_symmetry.cpp -- see query_symmetry.h
#include "query_symmetry.h"

#include <algorithm>

namespace gnnpe_host {

namespace {

struct AutSearch {
    const StaticGraph &q;
    std::vector<uint32_t> image;  // image[x] of the vertices assigned so far (0 .. depth-1)
    std::vector<uint8_t> used;

    bool edge(uint32_t a, uint32_t b) const
    {
        return std::binary_search(q.neighbors.begin() + q.offsets[a], q.neighbors.begin() + q.offsets[a + 1], b);
    }
    // may x go to y, given the images of 0 .. x-1?
    bool fits(uint32_t x, uint32_t y) const
    {
        if (used[y] || q.labels[x] != q.labels[y] || q.degree(x) != q.degree(y)) return false;
        for (uint32_t z = 0; z < x; z++)
            if (edge(x, z) != edge(y, image[z])) return false;
        return true;
    }
    // extend the map on 0 .. x-1 to an automorphism: true at the first one found
    bool extend(uint32_t x)
    {
        if (x == q.n) return true;
        for (uint32_t y = 0; y < q.n; y++) {
            if (!fits(x, y)) continue;
            image[x] = y;
            used[y] = 1;
            const bool found = extend(x + 1);
            used[y] = 0;
            if (found) return true;
        }
        return false;
    }
};

}  // namespace

QuerySymmetry query_symmetry(const StaticGraph &query)
{
    QuerySymmetry out;
    const uint32_t nq = query.n;
    AutSearch s{query, std::vector<uint32_t>(nq, 0), std::vector<uint8_t>(nq, 0)};
    for (uint32_t u = 0; u < nq; u++) {
        // 0 .. u-1 are fixed; an automorphism that fixes them takes u to some w >= u
        uint64_t orbit = 1;
        for (uint32_t w = u + 1; w < nq; w++) {
            if (!s.fits(u, w)) continue;
            s.image[u] = w;
            s.used[w] = 1;
            const bool found = s.extend(u + 1);
            s.used[w] = 0;
            if (found) {
                out.pairs.emplace_back(u, w);
                orbit++;
            }
        }
        out.n_automorphisms = out.n_automorphisms > ~0ull / orbit ? ~0ull : out.n_automorphisms * orbit;
        s.image[u] = u;
        s.used[u] = 1;
    }
    return out;
}

}  // namespace gnnpe_host
