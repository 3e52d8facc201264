// Swin shifted-window geometry (swin.py:90-255): the cyclic shift, the window partition and the shift mask are index arithmetic
// on the rolled map; the kernels that gather window tokens share it from here.
#pragma once
#include "common.h"

namespace mv {

struct WindowGeom {
    int Hf, Wf;      // feature map
    int wsh, wsw;    // window
    int shh, shw;    // cyclic shift (0 when the window covers the map)
};

// token t of window (wy, wx) -> its coordinates on the rolled map
__device__ __forceinline__ void swin_rolled(const WindowGeom& g, int wy, int wx, int t, int& y, int& x) {
    y = wy * g.wsh + t / g.wsw;
    x = wx * g.wsw + t % g.wsw;
}
// rolled (y, x) of image b -> the row of the [B, Hf, Wf] map it was rolled from: np.roll(x, -s)[i] = x[(i + s) % n]
// One conditional subtract IS the modulo: y < Hf, and a checked geometry (swin_check_geom) has shh < wsh <= Hf, so y + shh < 2 Hf.
__device__ __forceinline__ long long swin_src_row(const WindowGeom& g, int b, int y, int x) {
    int oy = y + g.shh, ox = x + g.shw;
    if (oy >= g.Hf) oy -= g.Hf;
    if (ox >= g.Wf) ox -= g.Wf;
    return ((long long)b * g.Hf + oy) * g.Wf + ox;
}
// shift-mask region id of rolled (y, x): 3 x 3 bands (swin.py:190-209); tokens of different regions do not attend to each other
__device__ __forceinline__ int swin_region(const WindowGeom& g, int y, int x) {
    const int rh = (y < g.Hf - g.wsh) ? 0 : (y < g.Hf - g.shh ? 1 : 2);
    const int rw = (x < g.Wf - g.wsw) ? 0 : (x < g.Wf - g.shw ? 1 : 2);
    return rh * 3 + rw;
}

// the two for token t of window (wy, wx)
__device__ __forceinline__ long long swin_tok_row(const WindowGeom& g, int b, int wy, int wx, int t) {
    int y, x;
    swin_rolled(g, wy, wx, t, y, x);
    return swin_src_row(g, b, y, x);
}
__device__ __forceinline__ int swin_tok_region(const WindowGeom& g, int wy, int wx, int t) {
    int y, x;
    swin_rolled(g, wy, wx, t, y, x);
    return swin_region(g, y, x);
}

// The argument check the window-attention entries share: heads divide C, the window divides the map, the shift is inside the
// window -- and is dropped where the window covers the map (swin.py:116-120).  Fills `g`; MV_OK or MV_E_INVALID with the error set.
inline int swin_check_geom(const char* who, int Hf, int Wf, int C, int heads, int ws_h, int ws_w, int shift_h, int shift_w,
                           WindowGeom& g) {
    if (C % heads != 0) {
        set_error("%s: C %% heads != 0", who);
        return MV_E_INVALID;
    }
    if (!(ws_h > 0 && ws_w > 0 && Hf % ws_h == 0 && Wf % ws_w == 0)) {
        set_error("%s: feature map %dx%d is not a multiple of the window %dx%d (reference swin.py:782-790)", who, Hf, Wf, ws_h, ws_w);
        return MV_E_INVALID;
    }
    if (!(shift_h >= 0 && shift_w >= 0 && shift_h < ws_h && shift_w < ws_w)) {
        set_error("%s: bad shift", who);
        return MV_E_INVALID;
    }
    g = {Hf, Wf, ws_h, ws_w, ws_h >= Hf ? 0 : shift_h, ws_w >= Wf ? 0 : shift_w};
    return MV_OK;
}

}  // namespace mv
