// The tile scheme of the a-trous units (psdr_jit_amd/csrc/hip/atrous.h): every workgroup and thread of the grid that level_grid() returns, walked on the host through the
// decode macros the kernels expand, for frames and strides at the tile's edges.  Every frame pixel has exactly one owner, no owner is outside the frame, a staged halo word
// is a frame pixel of the workgroup's coset, a tap's word lies inside the halo plane, and the tap masks say exactly which taps are inside the frame.
// Host compile only: g++ -O2 -std=c++17 -I<repo> tests/cpp/atrous_cover_check.cpp
#include <cstdio>
#include <vector>

#include "psdr_jit_amd/csrc/hip/atrous.h"

using namespace psdr::atrous;

static long failures = 0;
#define CHECK(cond) do { if (!(cond)) { if (failures < 20) std::printf("FAILED line %d: %s (W %d H %d s %d block %u %u)\n", __LINE__, #cond, F.W, F.H, F.s, block.x, block.y); ++failures; } } while (0)

struct Index { unsigned x, y; };         // stands in for blockIdx

static void walk_workgroup(const Frame &F, const Index &block, std::vector<int> &owners) {
    ATROUS_TILE(F, block, return);
    CHECK(n == F.W * F.H && a >= 0 && a < s && a < F.W && b >= 0 && b < s && b < F.H && wd >= 1 && hd >= 1);
    std::vector<int> staged(kHalo);               // the frame pixel staged in each halo word, -1: none
    for (int idx = 0; idx < kHalo; ++idx) {
        ATROUS_HALO_SLOT(F, idx);
        if (inside) CHECK(q >= 0 && q < n && (q % F.W) % s == a && (q / F.W) % s == b && q % F.W == a + hx * s && q / F.W == b + hy * s);
        else CHECK(q == 0);
        staged[idx] = inside ? q : -1;
    }
    auto walk_thread = [&](unsigned thread) {
        ATROUS_PIXEL(F, thread, return);
        const int x = a + dx * s, y = b + dy * s;
        CHECK(x >= 0 && x < F.W && y >= 0 && y < F.H && p == y * F.W + x);           // no owner outside the frame
        if (p >= 0 && p < n) ++owners[p];
        for (int j = -2; j <= 2; ++j)
            for (int i = -2; i <= 2; ++i) {
                const int slot = centre + j * kHX + i;
                CHECK(slot >= 0 && slot < kHalo);
                const bool in_frame = x + s * i >= 0 && x + s * i < F.W && y + s * j >= 0 && y + s * j < F.H;
                CHECK((okx[i + 2] && oky[j + 2]) == in_frame);
                if (slot >= 0 && slot < kHalo) CHECK(staged[slot] == (in_frame ? p + s * (j * F.W + i) : -1));      // the word a tap reads holds the tap's pixel
            }
    };
    for (unsigned thread = 0; thread < (unsigned) kThreads; ++thread) walk_thread(thread);
}

int main() {
    const int widths[] = {1, 5, 33, 67, 131}, heights[] = {1, 3, 9, 35, 127};
    long grids = 0;
    for (int W : widths)
        for (int H : heights)
            for (int l = 0; l < kMaxL; ++l) {
                Frame F{W, H, 1 << l, 0, 0};
                const Grid grid = level_grid(F);
                const Index block{grid.x, grid.y};          // (for CHECK's message)
                CHECK(grid.x >= 1 && grid.y >= 1 && grid.y <= 65535);
                std::vector<int> owners((size_t) W * H, 0);
                for (unsigned by = 0; by < grid.y; ++by)
                    for (unsigned bx = 0; bx < grid.x; ++bx) walk_workgroup(F, Index{bx, by}, owners);
                for (int p = 0; p < W * H; ++p) CHECK(owners[p] == 1);        // every pixel, exactly once
                ++grids;
            }
    if (failures) { std::printf("%ld check(s) failed\n", failures); return 1; }
    std::printf("OK: %ld grids\n", grids);
    return 0;
}
