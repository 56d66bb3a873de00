// bm_strip_plan.h — the strip kernel's launch geometry (bm_strip.hip): what it accepts, its LDS layout, which strips
// are interior and how many row bands each strip is cut into.
//
// The launcher passes what strip_lds and strip_grid compute.  The kernel shares the constants and stage_bytes, and
// keeps its LDS offsets and its interior test written out (through these functions its register allocation changes);
// tests/test_strip_plan.py holds the two to each other.  Host-only and free of HIP, so a plain C++ compiler builds it.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "bm_box_plan.h"

namespace sm {

constexpr int kSC = 128;      // input columns per strip
constexpr int kSP = kSC / 2;  // u16 column pairs per strip row
constexpr int kSQ = kSC / 4;  // 4-column groups per strip
constexpr int strip_out_cols(int R) { return kSC - 2 * R; }   // output columns per strip (SW)

// what the kernel takes: the plan's strip_path (bm_box_plan.h) and a known valid_mode
inline bool strip_args_ok(const BoxGeom& g, int valid_mode) {
    return strip_path(g) && g.batch > 0 && (valid_mode == 0 || valid_mode == 1);
}

// R staged words per copy of a row: columns rb0 .. rb0 + DP - d_lo + kSC + 3 (d_lo rounded down to 4; the lanes
// read staged columns DP - d .. DP - d + 127) as u16 pairs; copies r_stride words apart, = 16 mod 32, so that the
// lanes reading copy 0 (even DP - d) and copy 1 (odd) fall on disjoint halves of the banks
constexpr int r_words(int DP, int d_lo) { return (DP - (d_lo & ~3) + kSC + 4) / 2; }
constexpr int r_stride(int RW) { return ((RW + 15) & ~31) + 16; }
// one step's staging: L in/out as u16 column pairs, R in/out as two copies
constexpr int stage_bytes(int RS) { return 2 * kSP * 4 + 2 * 2 * RS * 4; }
// a step stages 2 kSQ + RW 4-column groups (L in, L out, R in, R out), each thread at most this many of them
constexpr int kStripStageItems = 3;

// LDS: [2] staging buffers, at wmin_off wmin [2][nw][8 ceil(SW / 8)] u32 (the waves' minima of a row), at rrow_off,
// with the right view, rrow [2][SW + DP] u32 (the row's right keys)
struct StripLds {
    int DP;       // d_hi - 1 rounded up to 4: staged R column DP - d + c holds strip column c's R(c - d)
    int RW, RS;   // r_words, r_stride
    int nw;       // waves: 64 disparities each
    int wmin_off, rrow_off, bytes;
};
constexpr StripLds strip_lds(int R, int d_lo, int d_hi, bool right) {
    StripLds l{};
    l.DP = ((d_hi - 1) + 3) & ~3;
    l.RW = r_words(l.DP, d_lo);
    l.RS = r_stride(l.RW);
    l.nw = (d_hi - d_lo + 63) / 64;
    l.wmin_off = 2 * stage_bytes(l.RS);
    l.rrow_off = l.wmin_off + 2 * l.nw * ((strip_out_cols(R) + 7) / 8) * 8 * 4;
    l.bytes = l.rrow_off + (right ? 2 * (strip_out_cols(R) + l.DP) * 4 : 0);
    return l;
}

// The strip with outputs x0 .. x0 + SW - 1 runs the unmasked body: every column of the strip >= every d and inside
// the frame (no AD masks), and every output inside the frame with every d valid (no key masks).
// valid_mode: 0 d <= W - x (Device.cu:44); 1 the mirrored right view's d <= x
constexpr bool strip_interior(int x0, int R, int W, int d_hi, int valid_mode) {
    const int SW = strip_out_cols(R), cs0 = x0 - R;
    const bool col_ok = cs0 >= d_hi - 1 && cs0 + kSC <= W;
    const bool out_ok = x0 + SW <= W && (valid_mode == 0 ? (d_hi - 1) <= W - (x0 + SW - 1) : (d_hi - 1) <= x0);
    return col_ok && out_ok;
}

struct StripGrid {
    int EL, NI, ER;   // left edge, interior and right edge strips: the interior strips are one contiguous run
    int nb, nbe;      // bands per interior / edge strip
};
// Row bands, one round of workgroups (a second, partial round would leave most of the chip idle while it runs):
// interior strips in nb bands, edge strips in nbe, chosen to minimise the longer of the two band walks, a band of
// height h costing (h + 2r) row steps (its first 2r steps only build V), an edge step kEdgeCost % of an
// interior one (the masked body), over the (nb, nbe) whose workgroups all fit `resident` at once; (1, 1) where none
// does.  Of equal walks the smallest nb, then the smallest nbe.  Sets s.nb and s.nbe from s.EL, s.NI and s.ER
constexpr int kEdgeCost = 150;
inline void strip_bands(StripGrid& s, int H, int R, int frames, int resident) {
    const int64_t ni = s.NI, ne = s.EL + s.ER;   // ne >= 1 in every frame: strip 0's left halo lies outside it
    const int nb_max = ni ? std::max(1, H / (4 * R)) : 1, nbe_max = ne ? std::max(1, H / (2 * R)) : 1;
    auto walk = [&](int64_t bands, int cost) { return ((H + bands - 1) / bands + 2 * R) * cost; };
    const int64_t room = resident / frames;   // workgroups per frame
    int64_t best = -1;
    for (int nb = 1; nb <= nb_max; ++nb) {
        // the edge walk only shortens with nbe, so this nb's best is at the most edge bands that fit, and the nbe to
        // take is the smallest whose walk is no longer than that best
        const int64_t left = room - ni * nb;   // workgroups per frame left to the edge strips
        int64_t cap = ne ? std::min<int64_t>(nbe_max, left / ne) : 1;
        if (left < 0 || cap < 1) {
            if (nb > 1) break;   // nor does any larger nb fit
            cap = 1;
        }
        const int64_t t = std::max<int64_t>(ni ? walk(nb, 100) : 0, ne ? walk(cap, kEdgeCost) : 0);
        if (best >= 0 && t >= best) continue;
        best = t;
        const int64_t h = t / kEdgeCost - 2 * R;   // the tallest edge band within t: (h + 2r) kEdgeCost <= t
        s.nb = nb;
        s.nbe = ne ? (int)((H + h - 1) / h) : 1;
    }
}
inline StripGrid strip_grid(const BoxGeom& g, int valid_mode, int resident) {
    const int SW = strip_out_cols(g.radius), strips = (g.W + SW - 1) / SW;
    StripGrid s{0, 0, 0, 1, 1};
    auto interior = [&](int st) { return strip_interior(st * SW, g.radius, g.W, g.d_hi, valid_mode); };
    while (s.EL < strips && !interior(s.EL)) ++s.EL;
    while (s.EL + s.NI < strips && interior(s.EL + s.NI)) ++s.NI;
    s.ER = strips - s.EL - s.NI;
    strip_bands(s, g.H, g.radius, g.batch, resident);
    return s;
}

}  // namespace sm
