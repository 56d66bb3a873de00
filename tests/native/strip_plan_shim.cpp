// C entries to csrc/bm_strip_plan.h, built with the host compiler alone, for tests/test_strip_plan.py.
#include "../../gpu_stereo_matching_amd/csrc/bm_strip_plan.h"

// out: EL, NI, ER, nb, nbe
extern "C" void strip_grid(int W, int H, int R, int d_lo, int d_hi, int valid_mode, int frames, int resident,
                           int out[5]) {
    const sm::StripGrid g = sm::strip_grid(sm::BoxGeom{W, H, W, R, d_lo, d_hi, frames}, valid_mode, resident);
    out[0] = g.EL, out[1] = g.NI, out[2] = g.ER, out[3] = g.nb, out[4] = g.nbe;
}

// out: nb, nbe
extern "C" void strip_bands(int ni, int ne, int H, int R, int frames, int resident, int out[2]) {
    sm::StripGrid s{0, ni, ne, 1, 1};
    sm::strip_bands(s, H, R, frames, resident);
    out[0] = s.nb, out[1] = s.nbe;
}

extern "C" int strip_interior(int x0, int R, int W, int d_hi, int valid_mode) {
    return sm::strip_interior(x0, R, W, d_hi, valid_mode);
}

extern "C" int strip_args_ok(int W, int H, int R, int d_lo, int d_hi, int batch, int valid_mode) {
    return sm::strip_args_ok(sm::BoxGeom{W, H, W, R, d_lo, d_hi, batch}, valid_mode);
}

// every slice 0 <= d_lo < d_hi <= 256 at radius R, d_lo-major: DP, RW, RS, nw, wmin_off, rrow_off, bytes, bytes of
// one staging buffer
extern "C" int strip_lds_all(int R, int right, int out[][8]) {
    int n = 0;
    for (int d_lo = 0; d_lo < sm::kStripMaxDisp; ++d_lo)
        for (int d_hi = d_lo + 1; d_hi <= sm::kStripMaxDisp; ++d_hi, ++n) {
            const sm::StripLds l = sm::strip_lds(R, d_lo, d_hi, right != 0);
            const int v[8] = {l.DP, l.RW, l.RS, l.nw, l.wmin_off, l.rrow_off, l.bytes, sm::stage_bytes(l.RS)};
            for (int i = 0; i < 8; ++i) out[n][i] = v[i];
        }
    return n;
}

extern "C" int strip_stage_items_per_thread() { return sm::kStripStageItems; }
