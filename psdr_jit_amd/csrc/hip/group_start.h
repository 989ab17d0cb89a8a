// group_start.h — when a wave of the interior term starts new samples, and which queue positions a start hands to which lane (paths.h::run_paths, MODE 0;
// tests/cpp/group_start_check.cpp plays a wave's loop with these functions on the host: g++ alone).
//
// A wave owns a local queue [next, end) of positions it took from the launch's queue (one atomic per kFetchBatch positions).  A start looks at the next 64 positions
// at once - a WINDOW, every lane one position -; the idle lanes take the live ones in order (lane order = position order), dead positions cost a bit test.  All of it
// is wave-uniform arithmetic on two 64-bit masks:
//     gs_start_now      the decision: at least G lanes idle, or nobody busy - and positions in hand
//     gs_window_len     the window's length at the queue's head
//     gs_lane_pick      the window position of one idle lane (-1: the window has fewer live positions than idle lanes below this one)
//     gs_window_used    the positions a window uses up: up to its last taken one, all of it when every live position found a lane
//     gs_fetched        the local queue after a fetch from the launch's queue
// Which position goes to which lane depends on the queue, the live bits and the idle mask only.
#pragma once

#if defined(__HIPCC__)
#define PSDR_GS_HD __host__ __device__ inline
#else
#define PSDR_GS_HD inline
#endif

namespace psdr {

PSDR_GS_HD int gs_popc(unsigned long long m) { return __builtin_popcountll(m); }

// position of the r-th (0-based) set bit of m; r < popcount(m)
PSDR_GS_HD int gs_nth_set_bit(unsigned long long m, int r) {
    unsigned w = (unsigned) m;
    int pos = 0;
    const int c0 = __builtin_popcount(w);
    if (r >= c0) { r -= c0; w = (unsigned) (m >> 32); pos = 32; }
    for (int half = 16; half >= 1; half >>= 1) {
        const int cl = __builtin_popcount(w & ((1u << half) - 1u));
        if (r >= cl) { r -= cl; w >>= half; pos += half; }
    }
    return pos;
}

// does the wave start samples in this loop iteration?  in_hand: its local queue holds positions (the caller fetches before it asks, so "none in hand" means
// the launch's queue is exhausted too: the wave only drains).  A wave whose lanes are all idle starts whatever G is - nobody waits on a start that cannot come
PSDR_GS_HD bool gs_start_now(int n_idle, int n_busy, int G, bool in_hand) { return n_idle > 0 && in_hand && (n_idle >= G || n_busy == 0); }

PSDR_GS_HD int gs_window_len(long long q_next, long long q_end) { return q_end - q_next < 64 ? (int) (q_end - q_next) : 64; }

// lv: the window's live positions; want: the lanes that still want a position; lt_mask: the lanes below this one
PSDR_GS_HD int gs_lane_pick(unsigned long long lv, unsigned long long want, unsigned long long lt_mask) {
    const int r = gs_popc(want & lt_mask);
    return r < gs_popc(lv) ? gs_nth_set_bit(lv, r) : -1;
}

PSDR_GS_HD int gs_window_used(unsigned long long lv, int n_want, int wlen) { return gs_popc(lv) <= n_want ? wlen : gs_nth_set_bit(lv, n_want - 1) + 1; }

// base: what the atomic on the launch's queue returned; n_local: the launch's positions
PSDR_GS_HD void gs_fetched(unsigned long long base, long long n_local, int batch, long long &q_next, long long &q_end, bool &exhausted) {
    if ((long long) base >= n_local) exhausted = true;
    else { q_next = (long long) base; q_end = q_next + batch < n_local ? q_next + batch : n_local; }
}

} // namespace psdr
