// C entries to csrc/bm_box_plan.h's tile queue (box_queue_grab, box_queue_grabs, box_queue_workgroups, the matrix-pipe kernel's tile counts), built with the host compiler alone, for tests/test_box_queue_plan.py.
#include "../../gpu_stereo_matching_amd/csrc/bm_box_plan.h"

extern "C" void box_queue_grab(unsigned g, unsigned total, unsigned tiles_x, unsigned slots, unsigned out[2]) {
    const sm::BoxGrab r = sm::box_queue_grab(g, total, tiles_x, slots);
    out[0] = r.begin;
    out[1] = r.end;
}

// Walks the grabs 0 .. n - 1 (n = box_queue_grabs) and the `past` grabs behind them in one call.  Returns 0 when
// they cover [0, total) in order without a gap, never grow, end with a single tile, and are empty past the end;
// else the 1-based number of the rule that failed.  out: n, the first and the largest grab's size, the grabs of
// one tile
extern "C" int box_queue_walk(unsigned total, unsigned tiles_x, unsigned slots, unsigned past, unsigned long long out[4]) {
    const unsigned n = sm::box_queue_grabs(total, tiles_x, slots);
    unsigned at = 0, prev = 0xFFFFFFFFu, first = 0, largest = 0, singles = 0;
    for (unsigned g = 0; g < n; ++g) {
        const sm::BoxGrab r = sm::box_queue_grab(g, total, tiles_x, slots);
        if (r.begin != at || r.end <= r.begin || r.end > total) return 1;
        const unsigned size = r.end - r.begin;
        if (size > prev) return 2;
        if (g == 0) first = size;
        if (size > largest) largest = size;
        singles += size == 1;
        prev = size;
        at = r.end;
    }
    if (at != total) return 3;
    if (n == 0 || prev != 1) return 4;
    for (unsigned g = n; g - n < past; ++g) {
        const sm::BoxGrab r = sm::box_queue_grab(g, total, tiles_x, slots);
        if (r.begin != r.end) return 5;
    }
    if (n >= 0x80000000u) return 6;
    out[0] = n;
    out[1] = first;
    out[2] = largest;
    out[3] = singles;
    return 0;
}

extern "C" int box_queue_workgroups(int np, int dspan, long long tiles, int slots, int workgroups, int queue_workgroups) {
    return sm::box_queue_workgroups(np, dspan, tiles, slots, workgroups, queue_workgroups);
}

extern "C" long long box_mfma_tiles(int W, int H, int radius, int dspan, int batch) {
    return sm::box_mfma_tiles(W, H, radius, dspan, batch);
}

extern "C" int box_queue_candidate(int W, int H, int radius, int d_lo, int d_hi, int batch, int valid_mode, int cus,
                                   int box_kernel, int workgroups, int queue_workgroups) {
    return sm::box_queue_candidate(sm::BoxGeom{W, H, W, radius, d_lo, d_hi, batch}, valid_mode, cus, box_kernel,
                                   workgroups, queue_workgroups);
}
