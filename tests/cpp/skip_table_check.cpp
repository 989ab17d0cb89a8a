// LaneRng::skip_levels (psdr_jit_amd/csrc/hip/sampler.h) against LaneRng::advance: the table of skip-ahead maps a path kernel applies when a
// path ends early must give the state the doubling loop gives, bit for bit - for every draw count per level (2, 3, 5), for every number of
// levels the table holds (1..kSkipLevelsMax) and for the larger ones, which take the loop.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../psdr_jit_amd/csrc/hip/sampler.h"

int main() {
    static_assert(psdr::kSkipLevelsMax == 8, "the cases below are written for a table of 8 levels");
    std::mt19937_64 gen(20240607u);
    long long checked = 0;
    const int nds[3] = {2, 3, 5};
    for (int nd : nds)
        for (int k = 1; k <= 12; ++k)
            for (int i = 0; i < 1000; ++i) {
                psdr::LaneRng a, b;
                a.state = b.state = gen();
                a.inc = b.inc = gen() | 1ull;
                a.advance((uint64_t) (nd * k));
                b.skip_levels(nd, k);
                if (a.state != b.state || a.inc != b.inc) {
                    std::printf("mismatch nd=%d k=%d state=%016llx want=%016llx\n", nd, k, (unsigned long long) b.state, (unsigned long long) a.state);
                    return 1;
                }
                // ... and the stream goes on with the same numbers
                if (a.next_u32() != b.next_u32()) { std::printf("mismatch after nd=%d k=%d\n", nd, k); return 1; }
                ++checked;
            }
    // the table's entries are skip_ahead's, which the launches already use for the sampler's draws so far
    const psdr::SkipLevels tab = psdr::make_skip_levels();
    for (int a = 0; a < 3; ++a)
        for (int k = 1; k <= psdr::kSkipLevelsMax; ++k) {
            const psdr::SkipAhead s = psdr::skip_ahead((uint64_t) (nds[a] * k));
            if (tab.e[a][k - 1].mult != s.mult || tab.e[a][k - 1].g != s.g) { std::printf("table entry nd=%d k=%d\n", nds[a], k); return 1; }
        }
    std::printf("ok %lld\n", checked);
    return 0;
}
