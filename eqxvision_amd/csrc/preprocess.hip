// Image preprocessing on the device, gfx950: uint8 images -> the float tensor the models read, in one launch.
// resize (separable triangle filter, half-pixel centres, antialiased when down-sampling) -> crop -> y = acc * a[c] + b[c].
// The filter lives in two tap tables the host builds in float64 (eqxvision_amd/preprocess.py: axis_table); the kernel only
// applies them, so the same entry serves the antialiased ImageNet preset and plain two-tap up-sampling.  HBM-bound gather, no
// matrix work: every input byte a tile needs is read once into LDS, both passes run out of LDS, every output is stored once.
// Five entries share the tile body (tile_rows); a launch has ONE tile and ONE LDS size, sized for the largest spans and pitches
// of its batch, so one steeply down-sampled image lowers the occupancy of the whole launch (accepted):
//   mv_preprocess_u8_fwd         one image size per launch, the two tables of the launch
//   mv_preprocess_u8_ragged_fwd  adds one record per image: a packed batch of any sizes, every image its own tables
//   mv_preprocess_u8_boxes_fwd   adds one box per image that is cropped FIRST and then resized, mirrored or not (the training
//                                transform); its filter is generated in the tile, no tables
//   mv_preprocess_u8_mix_fwd     adds to the boxes a partner per image mixed in, rectangles erased or replaced and the soft targets
//                                written alongside (mixup / cutmix / random erasing); a tile runs the passes once per image it needs
//   mv_preprocess_u8_seg_fwd     one window per image of the WHOLE image resized, mirrored and padded, the label map gathered
//                                alongside (the segmentation transform); the generated filter on the part of a tile that is not padding
// On the host every entry is its own argument rules, its loop over the host records, its parameter struct and one call, built from
//   check_args, check_buffers    B, sizes, dtype; no NULL buffer
//   check_image                  a record's image lies inside the packed buffer
//   check_taps                   the tap limit; the largest pitches of the batch
//   check_disjoint               no output overlaps an input or another output
//   prep_params, launch_tiles    the common parameters; tile and LDS sizing over the batch, the grid, the device status word, the
//                                launch.  The status word is fetched LAST in every entry (the three older ones used to fetch it before
//                                the tile was sized): without a device, a valid call whose geometry does not fit the LDS is told so.
// On the device the record kernels share image_inside (a record's image lies inside x), tile_of (the workgroup's tile) and the
// two table sources, tables_from_global and tables_resized.
#include "common.h"

namespace mv {

namespace {

// Table of one axis, n = cropped output extent, m = taps per output (the table's pitch): int32 first[n] | int32 count[n] |
// fp32 weight[n][m].  `first` indexes the INPUT axis; taps first .. first + count - 1 lie inside it.
struct PrepP {
    const uint8_t* x;
    void* y;
    const int* tab_h;
    const int* tab_w;
    const float* a;
    const float* b;
    unsigned* status;
    int Hin, Win, Hout, Wout, mh, mw;
    int TH, TW;                    // output tile
    int rows_cap, cols_cap, pitch; // staged input rectangle the LDS was sized for; bytes per staged line (multiple of 16)
};

// mv_preprocess_u8_ragged_fwd: one record per image (blockIdx.z) instead of one geometry per launch.  In `p`, x is the packed
// buffer, tab_h the packed table buffer, mh / mw / rows_cap / cols_cap / pitch the largest any image of the batch needs (what the
// LDS was sized for); Hin, Win and tab_w are not used.
struct PrepRaggedP {
    PrepP p;
    const mv_preprocess_image* rec;
    long long x_bytes, tab_words;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A record's image lies inside x: sizes >= 1, fewer than 2^31 bytes, `offset` within the x_bytes of the buffer.  The records are
// device data the host cannot see at launch time; a record that fails this forms no address at all.
template <class Record> __device__ __forceinline__ bool image_inside(const Record& g, long long x_bytes) {
    const long long img_bytes = (long long)g.Hin * g.Win * 3;
    return g.Hin >= 1 && g.Win >= 1 && img_bytes < (1LL << 31) && g.offset >= 0 && g.offset <= x_bytes - img_bytes;
}

// The TH x TW tile of the output this workgroup owns: its first row and column, its extent cut at the output's edge.
struct Tile {
    int y0, x0, th, tw;
};
__device__ __forceinline__ Tile tile_of(const PrepP& p) {
    const int y0 = blockIdx.y * p.TH, x0 = blockIdx.x * p.TW;
    return {y0, x0, min(p.TH, p.Hout - y0), min(p.TW, p.Wout - x0)};
}

// taps an n_in -> n_out resize can give one output: the open interval of half-width max(1, in / out), no more than the axis
__host__ __device__ inline int taps_needed(int in, int out_full) {
    const double ratio = (double)in / (double)out_full, sup = ratio > 1.0 ? ratio : 1.0;
    const double n = 2.0 * sup + 1.0;
    return n >= in ? in : (int)n;
}

// mv_preprocess_u8_boxes_fwd: one box per image (blockIdx.z), no tables.  In `p`, x is the packed buffer, mh / mw / rows_cap /
// cols_cap / pitch the largest any box of the batch needs; Hin, Win, tab_h and tab_w are not used.
struct PrepBoxesP {
    PrepP p;
    const mv_preprocess_box* rec;
    long long x_bytes;
};

// mv_preprocess_u8_seg_fwd: one record per image (blockIdx.z), no tables.  In `p`, x is the packed image buffer, Hout x Wout the
// window, mh / mw / rows_cap / cols_cap / pitch the largest any resize of the batch needs; Hin, Win, tab_h and tab_w are not used.
// m / labels: the packed masks and the int32 label maps, both NULL for an image-only launch.
struct PrepSegP {
    PrepP p;
    const mv_preprocess_seg* rec;
    const uint8_t* m;
    int* labels;
    long long x_bytes, m_bytes;
    int image_fill, mask_fill;
};

// The LDS of one tile: staged uint8 lines | fp32 horizontal sums | first / count of the tile's rows and columns | their weights.
struct TileLds {
    uint8_t* su8;
    float* sh;
    int *sfy, *sny, *sfx, *snx;
    float *swy, *swx;
};

// The input rectangle [r0, r1) x [c0, c1) a tile's taps touch; bad: something had to be cut to get there.
struct TileRect {
    int r0, r1, c0, c1, bad;
};

template <bool CHW_IN> __device__ __forceinline__ TileLds tile_lds(const PrepP& p) {
    extern __shared__ uint4 smem4[];
    const int lines_cap = CHW_IN ? 3 * p.rows_cap : p.rows_cap;
    TileLds L;
    L.su8 = (uint8_t*)smem4;
    L.sh = (float*)(L.su8 + (size_t)lines_cap * p.pitch);
    L.sfy = (int*)(L.sh + (size_t)p.rows_cap * 3 * p.TW);
    L.sny = L.sfy + p.TH;
    L.sfx = L.sny + p.TH;
    L.snx = L.sfx + p.TW;
    L.swy = (float*)(L.snx + p.TW);
    L.swx = L.swy + p.TH * p.mh;
    return L;
}

// Nothing that decides an address is trusted: the rectangle is cut to the image and to the LDS it was sized for, tap indices
// are clamped into it by the passes, and a source that needed either sets bit 2 of the device status word.
__device__ __forceinline__ void cut_rect(const PrepP& p, TileRect& t) {
    t.r0 = clampi(t.r0, 0, p.Hin - 1);
    t.c0 = clampi(t.c0, 0, p.Win - 1);
    t.r1 = clampi(t.r1, t.r0 + 1, p.Hin);
    t.c1 = clampi(t.c1, t.c0 + 1, p.Win);
    if (t.r1 - t.r0 > p.rows_cap) { t.r1 = t.r0 + p.rows_cap; t.bad = 1; }
    if (t.c1 - t.c0 > p.cols_cap) { t.c1 = t.c0 + p.cols_cap; t.bad = 1; }
    if (t.bad && threadIdx.x == 0) atomicOr(p.status, 4u);
}

// Step 1, source A: the tables of the tile's rows / columns from global memory (p.tab_h, p.tab_w).  The rectangle is uniform
// over the workgroup (scalar loads).  The tables are device data the host cannot see at launch time: see cut_rect.
__device__ __forceinline__ TileRect tables_from_global(const PrepP& p, const TileLds& L, int y0, int x0, int th, int tw) {
    const int tid = threadIdx.x;
    TileRect t = {p.Hin, 0, p.Win, 0, 0};
    for (int i = 0; i < th; ++i) {
        const int f = p.tab_h[y0 + i], n = p.tab_h[p.Hout + y0 + i];
        t.bad |= (f < 0) | (n < 1) | (n > p.mh) | (f + n > p.Hin);
        t.r0 = min(t.r0, f);
        t.r1 = max(t.r1, f + n);
    }
    for (int i = 0; i < tw; ++i) {
        const int f = p.tab_w[x0 + i], n = p.tab_w[p.Wout + x0 + i];
        t.bad |= (f < 0) | (n < 1) | (n > p.mw) | (f + n > p.Win);
        t.c0 = min(t.c0, f);
        t.c1 = max(t.c1, f + n);
    }
    cut_rect(p, t);
    for (int i = tid; i < th; i += 256) {
        L.sfy[i] = p.tab_h[y0 + i] - t.r0;
        L.sny[i] = clampi(p.tab_h[p.Hout + y0 + i], 1, p.mh);
    }
    for (int i = tid; i < tw; i += 256) {
        L.sfx[i] = p.tab_w[x0 + i] - t.c0;
        L.snx[i] = clampi(p.tab_w[p.Wout + x0 + i], 1, p.mw);
    }
    const float* wy = (const float*)(p.tab_h + 2 * (size_t)p.Hout) + (size_t)y0 * p.mh;
    for (int i = tid; i < th * p.mh; i += 256) L.swy[i] = wy[i];
    const float* wx = (const float*)(p.tab_w + 2 * (size_t)p.Wout) + (size_t)x0 * p.mw;
    for (int i = tid; i < tw * p.mw; i += 256) L.swx[i] = wx[i];
    return t;
}

// preprocess.axis_table(n_box, n_out) for output o, in float64 and without contraction, so that it is the same arithmetic as
// the host's: centre s, half-width sup, taps first .. last inside the box (box coordinates).
struct AxisTaps {
    double s, sup;
    int first, last;
};
__device__ __forceinline__ AxisTaps axis_taps(int n_box, int n_out, int o) {
#pragma clang fp contract(off)
    AxisTaps t;
    const double ratio = (double)n_box / (double)n_out;
    t.sup = ratio > 1.0 ? ratio : 1.0;
    t.s = ((double)o + 0.5) * ratio - 0.5;
    t.first = max((int)floor(t.s - t.sup) + 1, 0);
    t.last = min((int)ceil(t.s + t.sup) - 1, n_box - 1);
    return t;
}
__device__ __forceinline__ double axis_weight(const AxisTaps& t, int k) {
#pragma clang fp contract(off)
    return fmax(0.0, 1.0 - fabs((double)(t.first + k) - t.s) / t.sup);
}

// Step 1, generated: the filter of an h x w box at (top, left) of the image resized to Hr x Wr, for rows y0 .. y0 + th - 1 and
// columns x0 .. x0 + tw - 1 of the resized box.  Two uses: a box resized to the output itself, Hr x Wr = Hout x Wout and the tile
// a tile of the output (boxes, mix); the whole image, box (0, 0, Hin, Win), resized to Hr x Wr, of which the output is a window
// (seg, through tables_window).  Column j of a mirrored result is the unmirrored column Wr - 1 - j (same taps, same tap order).
// One thread per row or column of the tile: weights in ascending tap order, their sum accumulated in that order, each quotient
// rounded once to fp32.  first / last grow with the output, so the rectangle follows from the tile's extreme outputs (with a
// mirror the two column ends swap).  The caller has clamped the box into the image; counts are clamped to the pitches the launch
// was sized for.
__device__ __forceinline__ TileRect tables_resized(const PrepP& p, const TileLds& L, int top, int left, int h, int w, int Hr, int Wr,
                                                   int flip, int y0, int x0, int th, int tw) {
    const int tid = threadIdx.x;
    const int j0 = flip ? Wr - x0 - tw : x0;                 // the tile's unmirrored columns are j0 .. j0 + tw - 1
    TileRect t;
    t.r0 = top + axis_taps(h, Hr, y0).first;
    t.r1 = top + axis_taps(h, Hr, y0 + th - 1).last + 1;
    t.c0 = left + axis_taps(w, Wr, j0).first;
    t.c1 = left + axis_taps(w, Wr, j0 + tw - 1).last + 1;
    t.bad = 0;
    cut_rect(p, t);
    for (int i = tid; i < th + tw; i += 256) {
        const bool row = i < th;
        const int e = row ? i : i - th;
        const AxisTaps a = row ? axis_taps(h, Hr, y0 + e) : axis_taps(w, Wr, flip ? Wr - 1 - (x0 + e) : x0 + e);
        const int m = row ? p.mh : p.mw;
        const int n = clampi(a.last - a.first + 1, 1, m);
        double sum = 0.0;
        for (int k = 0; k < n; ++k) sum += axis_weight(a, k);
        float* dst = (row ? L.swy : L.swx) + e * m;
        for (int k = 0; k < n; ++k) dst[k] = (float)(axis_weight(a, k) / sum);
        (row ? L.sfy : L.sfx)[e] = row ? top + a.first - t.r0 : left + a.first - t.c0;
        (row ? L.sny : L.snx)[e] = n;
    }
    return t;
}

// The seg kernel's call: r0, q0 the resized row / mirrored column of the tile's first output, th_v x tw_v the prefix of the tile
// that lies inside Hr x Wr.  A forward, kept on purpose: with the call written out in the seg kernel its eight instantiations
// take two more VGPRs (the boxes and mix kernels call tables_resized directly at no such cost).
__device__ __forceinline__ TileRect tables_window(const PrepP& p, const TileLds& L, int Hr, int Wr, int flip, int r0, int q0,
                                                  int th_v, int tw_v) {
    return tables_resized(p, L, 0, 0, p.Hin, p.Win, Hr, Wr, flip, r0, q0, th_v, tw_v);
}

// Element `it` of a th x tw tile in store order: (row, channel, column) of the tile.
template <bool NHWC_OUT> __device__ __forceinline__ void tile_elem(const int it, const int tw, int& y, int& c, int& x) {
    if (NHWC_OUT) {
        const int yx = it / 3;
        c = it - yx * 3;
        y = yx / tw;
        x = yx - y * tw;
    } else {
        const int yc = it / tw;
        x = it - yc * tw;
        y = yc / 3;
        c = yc - y * 3;
    }
}

// v -> channel c of output pixel (Y, X) of image b of p.y; the one rounding of a bf16 output.
template <bool NHWC_OUT, bool BF16_OUT>
__device__ __forceinline__ void tile_store(const PrepP& p, const int b, const int Y, const int c, const int X, const float v) {
    const size_t o = NHWC_OUT ? (((size_t)b * p.Hout + Y) * p.Wout + X) * 3 + c : (((size_t)b * 3 + c) * p.Hout + Y) * p.Wout + X;
    if (BF16_OUT) ((bf16_t*)p.y)[o] = f2bf(v);
    else ((float*)p.y)[o] = v;
}

// One workgroup = one TH x TW tile of the cropped output of one image, all three channels.
//   1. the tables of the tile's rows / columns -> LDS, read from global memory or generated (the two sources above)
//   2. the input rectangle the tile's taps touch -> LDS as uint8, 16-byte global loads on 16-byte global addresses (a staged line
//      starts `address & 15` bytes into its LDS line); chunks that would cross the ends of the image go byte by byte
//   3. horizontal pass: every staged row x tile column x channel -> fp32 LDS
//   4. vertical pass + affine epilogue -> global
// Each pass sums about the smallest of its taps, sum_k w[k] (v[k] - vmin) + vmin, as fp32 fmas in tap order.  The weights of an
// output sum to 1, so this is the same filter, and it buys two things over sum_k w[k] v[k]: every term and every partial sum is
// >= 0 and <= the result, so the rounding error is bounded by (taps + 1) 2^-24 of the result itself whatever the image; and a
// constant neighbourhood comes out as that constant exactly, however the fp32 weights happen to round (a flat image gives
// fma(v, a, b) bit for bit, borders included).  Nothing is shared between workgroups: two runs give the same bits.
// Steps 2 - 4.  `img`: the first byte of the image, whose size is p's; `t`: the rectangle step 1 left; sink(y, c, x, v) receives the
// fp32 value of every element of the tile, in store order, before any output rounding.
template <bool CHW_IN, bool NHWC_OUT, class Sink>
__device__ __forceinline__ void tile_rows(const PrepP& p, const TileLds& L, const TileRect& t, const uint8_t* img, const int th,
                                          const int tw, Sink&& sink) {
    const int tid = threadIdx.x;
    constexpr int PIX = CHW_IN ? 1 : 3;                      // bytes from one pixel of a channel to the next
    uint8_t* su8 = L.su8;
    float* sh = L.sh;
    const int *sfy = L.sfy, *sny = L.sny, *sfx = L.sfx, *snx = L.snx;
    const float *swy = L.swy, *swx = L.swx;
    const int r0 = t.r0, c0 = t.c0, nrows = t.r1 - t.r0, ncols = t.c1 - t.c0;

    // 2. input rectangle
    const size_t img_bytes = (size_t)p.Hin * p.Win * 3;
    const uintptr_t img_lo = (uintptr_t)img, img_hi = img_lo + img_bytes;
    const int lines = CHW_IN ? 3 * nrows : nrows;
    const int len = ncols * PIX;
    const int nch = p.pitch >> 4;
    auto line_addr = [&](int l) -> uintptr_t {
        if (CHW_IN) {
            const int c = l / nrows, r = r0 + (l - c * nrows);
            return img_lo + ((size_t)c * p.Hin + r) * p.Win + c0;
        }
        return img_lo + ((size_t)(r0 + l) * p.Win + c0) * 3;
    };
    for (int it = tid; it < lines * nch; it += 256) {
        const int l = it / nch, j = it - l * nch;
        const uintptr_t g = line_addr(l);
        const uintptr_t ca = (g & ~(uintptr_t)15) + 16 * (uintptr_t)j;
        if (ca >= g + len) continue;
        uint8_t* d = su8 + (size_t)l * p.pitch + 16 * j;
        if (ca >= img_lo && ca + 16 <= img_hi) {
            *(uint4*)d = *(const uint4*)ca;
        } else {                                             // ragged head of the first line / tail of the last line of the image
            for (int k = 0; k < 16; ++k)
                if (ca + k >= img_lo && ca + k < img_hi) d[k] = *(const uint8_t*)(ca + k);
        }
    }
    __syncthreads();

    // 3. horizontal pass: sh[(r * 3 + c) * TW + x]
    for (int it = tid; it < nrows * 3 * tw; it += 256) {
        const int rc = it / tw, x = it - rc * tw;
        const int r = rc / 3, c = rc - r * 3;
        const int l = CHW_IN ? c * nrows + r : r;
        const uint8_t* src = su8 + (size_t)l * p.pitch + (int)(line_addr(l) & 15) + (CHW_IN ? 0 : c);
        const int f = sfx[x], n = snx[x];
        const float* w = swx + x * p.mw;
        int m = 255;
        for (int k = 0; k < n; ++k) m = min(m, (int)src[clampi(f + k, 0, ncols - 1) * PIX]);
        float acc = 0.f;
        for (int k = 0; k < n; ++k) acc = fmaf(w[k], (float)((int)src[clampi(f + k, 0, ncols - 1) * PIX] - m), acc);
        sh[rc * p.TW + x] = acc + (float)m;
    }
    __syncthreads();

    // 4. vertical pass, epilogue, store
    const float a0 = p.a[0], a1 = p.a[1], a2 = p.a[2], b0 = p.b[0], b1 = p.b[1], b2 = p.b[2];
    for (int it = tid; it < th * 3 * tw; it += 256) {
        int y, c, x;
        tile_elem<NHWC_OUT>(it, tw, y, c, x);
        const int f = sfy[y], n = sny[y];
        const float* w = swy + y * p.mh;
        float m = sh[(clampi(f, 0, nrows - 1) * 3 + c) * p.TW + x];
        for (int k = 1; k < n; ++k) m = fminf(m, sh[(clampi(f + k, 0, nrows - 1) * 3 + c) * p.TW + x]);
        float acc = 0.f;
        for (int k = 0; k < n; ++k) acc = fmaf(w[k], sh[(clampi(f + k, 0, nrows - 1) * 3 + c) * p.TW + x] - m, acc);
        acc += m;
        sink(y, c, x, fmaf(acc, c == 0 ? a0 : (c == 1 ? a1 : a2), c == 0 ? b0 : (c == 1 ? b1 : b2)));
    }
}

// Steps 2 - 4 with the plain store: the tile of image b of p.y.
template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__device__ __forceinline__ void tile_passes(const PrepP& p, const TileLds& L, const TileRect& t, const uint8_t* img, const int b,
                                            const int y0, const int x0, const int th, const int tw) {
    tile_rows<CHW_IN, NHWC_OUT>(p, L, t, img, th, tw, [&](const int y, const int c, const int x, const float v) {
        tile_store<NHWC_OUT, BF16_OUT>(p, b, y0 + y, c, x0 + x, v);
    });
}


template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__device__ __forceinline__ void preprocess_tile(const PrepP& p, const uint8_t* img, const int b) {
    const Tile o = tile_of(p);
    const TileLds L = tile_lds<CHW_IN>(p);
    const TileRect t = tables_from_global(p, L, o.y0, o.x0, o.th, o.tw);
    tile_passes<CHW_IN, NHWC_OUT, BF16_OUT>(p, L, t, img, b, o.y0, o.x0, o.th, o.tw);
}

template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const PrepP p) {
    const int b = blockIdx.z;
    preprocess_tile<CHW_IN, NHWC_OUT, BF16_OUT>(p, p.x + (size_t)b * ((size_t)p.Hin * p.Win * 3), b);
}

// The record is device data like the tables: the host validated its own copy, the kernel trusts neither.  A record whose image
// or tables would leave their buffers, or whose table pitch exceeds what the LDS was sized for, forms no address at all: its
// tiles store nothing and set bit 2.  (Uniform over the workgroup, before any barrier.)  A record that passes describes memory
// inside the two buffers, and the tile body cuts everything else -- rectangle, taps -- as it does for the tables.
template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__global__ __launch_bounds__(256) void preprocess_u8_ragged_kernel(const PrepRaggedP r) {
    const int b = blockIdx.z;
    const mv_preprocess_image g = r.rec[b];
    PrepP p = r.p;
    const bool ok = image_inside(g, r.x_bytes) && g.mh >= 1 && g.mh <= p.mh && g.mw >= 1 && g.mw <= p.mw &&
                    g.tab_h >= 0 && g.tab_w >= 0 && (long long)g.tab_h + (long long)p.Hout * (2 + g.mh) <= r.tab_words &&
                    (long long)g.tab_w + (long long)p.Wout * (2 + g.mw) <= r.tab_words;
    if (!ok) {
        if (threadIdx.x == 0) atomicOr(p.status, 4u);
        return;
    }
    p.Hin = g.Hin; p.Win = g.Win; p.mh = g.mh; p.mw = g.mw;
    p.tab_w = p.tab_h + g.tab_w;
    p.tab_h = p.tab_h + g.tab_h;
    preprocess_tile<CHW_IN, NHWC_OUT, BF16_OUT>(p, p.x + g.offset, b);
}

// The box record is device data too.  A record whose image would leave x forms no address: its tiles store nothing.  A box that
// leaves its image is clamped into it, and a box that needs more taps than the launch's pitches has its counts clamped (in
// tables_resized); each of these sets bit 2.  (Uniform over the workgroup, before any barrier.)
struct BoxSrc {
    const uint8_t* img;
    int Hin, Win, top, left, h, w, flip;
    bool ok, cut;       // ok: the image lies inside x (else nothing of the record is used); cut: the box or its taps had to be clamped
};
__device__ __forceinline__ BoxSrc box_source(const PrepP& p, const mv_preprocess_box& g, const long long x_bytes) {
    BoxSrc s;
    s.ok = image_inside(g, x_bytes);
    s.img = p.x + (s.ok ? g.offset : 0);
    s.Hin = g.Hin; s.Win = g.Win; s.flip = g.flip != 0;
    s.top = clampi(g.top, 0, g.Hin - 1); s.left = clampi(g.left, 0, g.Win - 1);
    s.h = clampi(g.h, 1, g.Hin - s.top); s.w = clampi(g.w, 1, g.Win - s.left);
    s.cut = s.top != g.top || s.left != g.left || s.h != g.h || s.w != g.w || taps_needed(s.h, p.Hout) > p.mh ||
            taps_needed(s.w, p.Wout) > p.mw;
    return s;
}

template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__global__ __launch_bounds__(256) void preprocess_u8_boxes_kernel(const PrepBoxesP r) {
    const int b = blockIdx.z;
    PrepP p = r.p;
    const BoxSrc s = box_source(p, r.rec[b], r.x_bytes);
    if (!s.ok) {
        if (threadIdx.x == 0) atomicOr(p.status, 4u);
        return;
    }
    p.Hin = s.Hin; p.Win = s.Win;
    if (s.cut && threadIdx.x == 0) atomicOr(p.status, 4u);
    const Tile o = tile_of(p);
    const TileLds L = tile_lds<CHW_IN>(p);
    const TileRect t = tables_resized(p, L, s.top, s.left, s.h, s.w, p.Hout, p.Wout, s.flip, o.y0, o.x0, o.th, o.tw);
    tile_passes<CHW_IN, NHWC_OUT, BF16_OUT>(p, L, t, s.img, b, o.y0, o.x0, o.th, o.tw);
}

// mv_preprocess_u8_mix_fwd.  The image workgroups (blockIdx.z < B): one tile of image b as in the boxes kernel, where every
// element is a function of v_i (this image through its own box) and v_r (its partner through the partner's box):
//     v_i = 0 inside image b's erase rectangle, v_r = 0 inside the PARTNER's;
//     inside the cut rectangle v_r; else, without a partner or with lam == 1, v_i; else fadd(fmul(lam, v_i), fmul(oml, v_r)).
// Which of the two resamples a tile runs is decided per tile from the records (uniform over the workgroup, before any barrier):
//     v_r is needed  unless there is no partner, or lam == 1 and the tile lies wholly outside the cut rectangle;
//     v_i is needed  unless there is a partner and the tile lies wholly inside the cut rectangle;
//     a needed value whose erase rectangle holds the whole tile is 0 without staging its image.
// A tile that runs both keeps the partner's th x tw x 3 fp32 values in LDS (`sv`, behind the tables: the launch was sized for it
// when the host records hold a partner, `keep`) while the passes run again on its own window: the two staged windows are never
// resident together.  The records are device data: a partner outside [0, B), a partner whose image leaves x, or a partner the
// launch has no `sv` for is treated as none, rectangles are clamped to the output; each sets bit 2.
// The target workgroups (blockIdx.z >= B) write targets[i][k] = fadd(fmul(lam_t, s(labels[i], k)), fmul(oml_t, s(labels[r], k))),
// s(y, k) = k == y ? on : off, grid-stride over B * K; a label outside [0, K) matches no k (off everywhere) and sets bit 3.
struct PrepMixP {
    PrepP p;
    const mv_preprocess_box* rec;
    const mv_preprocess_mix* mix;
    long long x_bytes;
    const int* labels;
    float* targets;
    int B, K, keep;
    float on, off;
};

struct OutRect {
    int y0, x0, y1, x1;
};
__device__ __forceinline__ OutRect out_rect(const PrepP& p, int y0, int x0, int y1, int x1, bool& bad) {
    const OutRect r = {clampi(y0, 0, p.Hout), clampi(x0, 0, p.Wout), clampi(y1, 0, p.Hout), clampi(x1, 0, p.Wout)};
    bad |= r.y0 != y0 || r.x0 != x0 || r.y1 != y1 || r.x1 != x1;
    return r;
}
__device__ __forceinline__ bool rect_has(const OutRect& r, int Y, int X) { return Y >= r.y0 && Y < r.y1 && X >= r.x0 && X < r.x1; }
// the non-empty tile t lies wholly inside r / shares a pixel with r
__device__ __forceinline__ bool rect_holds(const OutRect& r, const Tile& t) {
    return r.y0 <= t.y0 && t.y0 + t.th <= r.y1 && r.x0 <= t.x0 && t.x0 + t.tw <= r.x1;
}
__device__ __forceinline__ bool rect_meets(const OutRect& r, const Tile& t) {
    return max(r.y0, t.y0) < min(r.y1, t.y0 + t.th) && max(r.x0, t.x0) < min(r.x1, t.x0 + t.tw);
}

__device__ __forceinline__ void mix_targets(const PrepMixP& r) {
    const long long nthr = (long long)gridDim.x * gridDim.y * (gridDim.z - r.B) * 256;
    const long long first = (((long long)(blockIdx.z - r.B) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const long long total = (long long)r.B * r.K;
    unsigned bits = 0;
    for (long long e = first; e < total; e += nthr) {
        const int i = (int)(e / r.K), k = (int)(e - (long long)i * r.K);
        int pr = r.mix[i].partner;
        if (pr < 0 || pr >= r.B) { pr = i; bits |= 4u; }
        const int yi = r.labels[i], yr = r.labels[pr];
        if (yi < 0 || yi >= r.K || yr < 0 || yr >= r.K) bits |= 8u;
        r.targets[e] = mul_add_rn(r.mix[i].lam_t, k == yi ? r.on : r.off, r.mix[i].oml_t, k == yr ? r.on : r.off);
    }
    if (bits) atomicOr(r.p.status, bits);
}

template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__global__ __launch_bounds__(256) void preprocess_u8_mix_kernel(const PrepMixP r) {
    if ((int)blockIdx.z >= r.B) {
        mix_targets(r);
        return;
    }
    const int b = blockIdx.z;
    const PrepP& p = r.p;
    const BoxSrc own = box_source(p, r.rec[b], r.x_bytes);
    if (!own.ok) {
        if (threadIdx.x == 0) atomicOr(p.status, 4u);
        return;
    }
    const mv_preprocess_mix m = r.mix[b];
    bool bad = own.cut;
    int pr = m.partner;
    if (pr < 0 || pr >= r.B || (pr != b && !r.keep)) { pr = b; bad = true; }
    BoxSrc par = own;
    if (pr != b) {
        par = box_source(p, r.rec[pr], r.x_bytes);
        if (!par.ok) { pr = b; par = own; bad = true; }
        bad |= par.cut;
    }
    const bool mixed = pr != b;
    const OutRect cut = out_rect(p, m.cy0, m.cx0, m.cy1, m.cx1, bad);
    const OutRect er_i = out_rect(p, m.ey0, m.ex0, m.ey1, m.ex1, bad);
    OutRect er_r = er_i;
    if (mixed) {
        const mv_preprocess_mix mr = r.mix[pr];
        er_r = out_rect(p, mr.ey0, mr.ex0, mr.ey1, mr.ex1, bad);
    }
    if (bad && threadIdx.x == 0) atomicOr(p.status, 4u);
    const float lam = m.lam, oml = m.oml;

    const Tile o = tile_of(p);
    const bool need_r = mixed && (lam != 1.f || rect_meets(cut, o));
    const bool need_i = !(mixed && rect_holds(cut, o));
    const bool run_r = need_r && !rect_holds(er_r, o);
    const bool run_i = need_i && !rect_holds(er_i, o);

    auto emit = [&](const int y, const int c, const int x, float vi, float vr) {
        const int Y = o.y0 + y, X = o.x0 + x;
        if (rect_has(er_i, Y, X)) vi = 0.f;
        if (rect_has(er_r, Y, X)) vr = 0.f;
        float v;
        if (mixed && rect_has(cut, Y, X)) v = vr;
        else if (!mixed || lam == 1.f) v = vi;
        else v = mul_add_rn(lam, vi, oml, vr);
        tile_store<NHWC_OUT, BF16_OUT>(p, b, Y, c, X, v);
    };
    const TileLds L = tile_lds<CHW_IN>(p);
    float* sv = L.swx + p.TW * p.mw;                         // [th][3][TW] of v_r, only where the launch has `keep`
    auto resample = [&](const BoxSrc& s, auto&& sink) {
        PrepP q = p;
        q.Hin = s.Hin; q.Win = s.Win;
        const TileRect t = tables_resized(q, L, s.top, s.left, s.h, s.w, q.Hout, q.Wout, s.flip, o.y0, o.x0, o.th, o.tw);
        tile_rows<CHW_IN, NHWC_OUT>(q, L, t, s.img, o.th, o.tw, sink);
    };
    if (run_r && run_i) {
        resample(par, [&](const int y, const int c, const int x, const float v) { sv[(y * 3 + c) * p.TW + x] = v; });
        __syncthreads();                                     // the tables and sums of the partner's passes are rewritten next
        resample(own, [&](const int y, const int c, const int x, const float v) { emit(y, c, x, v, sv[(y * 3 + c) * p.TW + x]); });
    } else if (run_r) {
        resample(par, [&](const int y, const int c, const int x, const float v) { emit(y, c, x, 0.f, v); });
    } else if (run_i) {
        resample(own, [&](const int y, const int c, const int x, const float v) { emit(y, c, x, v, 0.f); });
    } else {
        for (int it = threadIdx.x; it < o.th * 3 * o.tw; it += 256) {
            int y, c, x;
            tile_elem<NHWC_OUT>(it, o.tw, y, c, x);
            emit(y, c, x, 0.f, 0.f);
        }
    }
}

// The elements of a th x tw tile outside its valid th_v x tw_v prefix <- v[c], in the store order of tile_passes' step 4.
template <bool NHWC_OUT, bool BF16_OUT>
__device__ __forceinline__ void tile_fill(const PrepP& p, const int b, const int y0, const int x0, const int th, const int tw,
                                          const int th_v, const int tw_v, const float v0, const float v1, const float v2) {
    for (int it = threadIdx.x; it < th * 3 * tw; it += 256) {
        int y, c, x;
        tile_elem<NHWC_OUT>(it, tw, y, c, x);
        if (y < th_v && x < tw_v) continue;
        tile_store<NHWC_OUT, BF16_OUT>(p, b, y0 + y, c, x0 + x, c == 0 ? v0 : (c == 1 ? v1 : v2));
    }
}

// The seg record is device data too.  A record whose image or mask would leave its buffer forms no address: its tiles store
// nothing.  The resized size is raised to 1 x 1, the window origin is clamped into the padded image max(Hr, Hout) x max(Wr, Wout),
// and a resize that needs more taps than the launch's pitches has its counts clamped (in tables_resized); each of these sets bit
// 2.  (Uniform over the workgroup, before any barrier.)  The padding is a suffix of rows and columns, so the part of a tile that
// lies inside the resized image is a prefix th_v x tw_v: that prefix goes through the tile body, the rest of the tile is the fill,
// and a tile that lies wholly in the padding stages nothing.  Labels: one thread per output pixel of the tile, rows of int32.
template <bool CHW_IN, bool NHWC_OUT, bool BF16_OUT>
__global__ __launch_bounds__(256) void preprocess_u8_seg_kernel(const PrepSegP r) {
    const int b = blockIdx.z;
    const mv_preprocess_seg g = r.rec[b];
    PrepP p = r.p;
    const long long px = (long long)g.Hin * g.Win;        // image_inside written out: through it these instantiations lose an SGPR
    const bool ok = g.Hin >= 1 && g.Win >= 1 && px * 3 < (1LL << 31) && g.offset >= 0 && g.offset <= r.x_bytes - px * 3 &&
                    (!r.m || (g.mask_offset >= 0 && g.mask_offset <= r.m_bytes - px));
    if (!ok) {
        if (threadIdx.x == 0) atomicOr(p.status, 4u);
        return;
    }
    p.Hin = g.Hin; p.Win = g.Win;
    const int Hr = max(g.Hr, 1), Wr = max(g.Wr, 1);
    const int top = clampi(g.top, 0, max(Hr, p.Hout) - p.Hout), left = clampi(g.left, 0, max(Wr, p.Wout) - p.Wout);
    const bool cut = Hr != g.Hr || Wr != g.Wr || top != g.top || left != g.left || taps_needed(g.Hin, Hr) > p.mh ||
                     taps_needed(g.Win, Wr) > p.mw;
    if (cut && threadIdx.x == 0) atomicOr(p.status, 4u);
    const int flip = g.flip != 0;
    const Tile o = tile_of(p);
    const int y0 = o.y0, x0 = o.x0, th = o.th, tw = o.tw;
    const int r0 = top + y0, q0 = left + x0;                 // < max(Hr, Hout), max(Wr, Wout): no overflow
    const int th_v = clampi(Hr - r0, 0, th), tw_v = clampi(Wr - q0, 0, tw);
    if (th_v > 0 && tw_v > 0) {
        const TileLds L = tile_lds<CHW_IN>(p);
        const TileRect t = tables_window(p, L, Hr, Wr, flip, r0, q0, th_v, tw_v);
        tile_passes<CHW_IN, NHWC_OUT, BF16_OUT>(p, L, t, p.x + g.offset, b, y0, x0, th_v, tw_v);
    }
    if (th_v < th || tw_v < tw) {
        const float f = (float)r.image_fill;
        tile_fill<NHWC_OUT, BF16_OUT>(p, b, y0, x0, th, tw, th_v, tw_v, fmaf(f, p.a[0], p.b[0]), fmaf(f, p.a[1], p.b[1]),
                                      fmaf(f, p.a[2], p.b[2]));
    }
    if (!r.labels) return;
    const uint8_t* mask = r.m + g.mask_offset;
    for (int it = threadIdx.x; it < th * tw; it += 256) {
        const int i = it / tw, j = it - i * tw;
        int v = r.mask_fill;
        if (i < th_v && j < tw_v) {
            const int q = q0 + j, cr = flip ? Wr - 1 - q : q;
            const long long sr = ((2LL * (r0 + i) + 1) * g.Hin) / (2LL * Hr), sc = ((2LL * cr + 1) * g.Win) / (2LL * Wr);
            v = mask[min(sr, (long long)g.Hin - 1) * g.Win + min(sc, (long long)g.Win - 1)];
        }
        r.labels[((size_t)b * p.Hout + y0 + i) * p.Wout + x0 + j] = v;
    }
}

// input samples a run of T outputs can touch on one axis: (T - 1) * ratio between the first and the last centre, the support on
// both sides, one for the inclusive end, one for rounding
int span_cap(int T, int in, int out_full) {
    const double ratio = (double)in / (double)out_full, sup = ratio > 1.0 ? ratio : 1.0;
    const double s = (T - 1) * ratio + 2.0 * sup + 2.0;
    return s >= in ? in : (int)s;
}

size_t lds_bytes(int TH, int TW, int rows_cap, int cols_cap, int in_chw, int mh, int mw, int* pitch) {
    const int pix = in_chw ? 1 : 3;
    *pitch = (cols_cap * pix + 15 + 15) & ~15;
    const size_t lines = in_chw ? 3 * (size_t)rows_cap : rows_cap;
    return lines * *pitch + (size_t)rows_cap * 3 * TW * 4 + (size_t)(2 * TH + 2 * TW + TH * mh + TW * mw) * 4;
}

// Tile: the largest of these whose staged rectangle fits 64 KiB of LDS.  The ImageNet preset on a 500 x 375 image (ratio
// 1.46) takes 32 x 32: 51 input rows x 51 columns staged = 51 x 176 B of uint8 + 51 x 3 x 32 fp32 of horizontal sums + 1.3 KiB
// of tables = 29.9 KiB -> 5 workgroups of 4 waves per CU = 5 waves per SIMD, 49 tiles per image.  Smaller tiles keep steep
// down-sampling (up to 11.5x, 24 taps) inside the budget; their stores are shorter runs, which such a reduction can afford.
// caps(TH, TW, &rows, &cols): the input rectangle a TH x TW tile can need.  p.mh / p.mw are read; TH, TW, rows_cap, cols_cap and
// pitch of the chosen tile (or of the smallest, if none fits) are left in p, its LDS size in *lds.
// keep: the tile also holds TH x 3 x TW fp32 results behind its tables (mv_preprocess_u8_mix_fwd: the partner's values).
template <class F> bool pick_tile(PrepP& p, int in_chw, size_t* lds, F&& caps, bool keep = false) {
    static const int tiles[][2] = {{32, 32}, {16, 32}, {16, 16}, {8, 16}, {4, 8}};
    for (const auto& t : tiles) {
        p.TH = t[0];
        p.TW = t[1];
        caps(p.TH, p.TW, &p.rows_cap, &p.cols_cap);
        *lds = lds_bytes(p.TH, p.TW, p.rows_cap, p.cols_cap, in_chw, p.mh, p.mw, &p.pitch) + (keep ? (size_t)p.TH * 3 * p.TW * 4 : 0);
        if (*lds <= 64 * 1024) return true;
    }
    return false;
}

// ---- what the five entries share on the host.  `who` is the entry's name in every message. ----

// The arguments every entry takes: B in (0, max_B], positive sizes (`sizes_ok`: the entry's own), an output dtype.  `image`: the
// one image size {Hin, Win} of the plain entry, whose "too large" line covers it too.
int check_args(const char* who, bool sizes_ok, int out_dtype, int B, int max_B, const int* image = nullptr) {
    MV_CHECK_ARG(B > 0 && sizes_ok, "%s: bad sizes", who);
    MV_CHECK_ARG(out_dtype == MV_F32 || out_dtype == MV_BF16, "%s: out_dtype must be MV_F32 or MV_BF16", who);
    if (image)
        MV_CHECK_ARG(B <= max_B && (long long)image[0] * image[1] * 3 < (1LL << 31), "%s: batch %d or image %dx%d too large", who, B,
                     image[0], image[1]);
    else
        MV_CHECK_ARG(B <= max_B, "%s: batch %d too large", who, B);
    return MV_OK;
}

int check_buffers(const char* who, std::initializer_list<const void*> buffers) {
    for (const void* v : buffers)
        if (!v) {
            set_error("%s: null buffer", who);
            return MV_E_UNSUPPORTED;
        }
    return MV_OK;
}

// Image i of a host record: positive sizes (`sizes_ok`: the record's other ones), fewer than 2^31 bytes, inside the x_bytes of x.
int check_image(const char* who, int i, int Hin, int Win, bool sizes_ok, int64_t offset, int64_t x_bytes) {
    MV_CHECK_ARG(Hin > 0 && Win > 0 && sizes_ok, "%s: image %d: bad sizes", who, i);
    const long long img_bytes = (long long)Hin * Win * 3;
    MV_CHECK_ARG(img_bytes < (1LL << 31), "%s: image %d: %dx%d too large", who, i, Hin, Win);
    MV_CHECK_ARG(offset >= 0 && offset <= x_bytes - img_bytes, "%s: image %d: %lld bytes at offset %lld do not lie inside the buffer of %lld bytes",
                 who, i, img_bytes, (long long)offset, (long long)x_bytes);
    return MV_OK;
}

// The tap limit of an in_h x in_w -> out_h x out_w resize (`what`: "" or "box "), of image i or, i < 0, of the launch.  `tables`:
// the pitches {mh, mw} of tables the caller brought, which obey the limit too and are named in the refusal.  *mh, *mw are
// raised to what this resize needs: the pitches of its tables, or the taps the kernel will generate.
int check_taps(const char* who, int i, const char* what, int in_h, int in_w, int out_h, int out_w, const int* tables, int* mh, int* mw) {
    const int need_h = taps_needed(in_h, out_h), need_w = taps_needed(in_w, out_w);
    const int pitch_h = tables ? tables[0] : need_h, pitch_w = tables ? tables[1] : need_w;
    if (std::max(std::max(need_h, need_w), std::max(pitch_h, pitch_w)) > MV_PREPROCESS_MAX_TAPS) {
        char image[32] = "", brought[48] = "";
        if (i >= 0) snprintf(image, sizeof(image), "image %d: ", i);
        if (tables) snprintf(brought, sizeof(brought), " (tables of %d x %d)", pitch_h, pitch_w);
        set_error("%s: %s%s%dx%d -> %dx%d needs up to %d x %d taps%s; at most %d per axis (down-sampling by up to %.1f)", who, image, what,
                  in_h, in_w, out_h, out_w, need_h, need_w, brought, MV_PREPROCESS_MAX_TAPS, (MV_PREPROCESS_MAX_TAPS - 1) / 2.0);
        return MV_E_UNSUPPORTED;
    }
    *mh = std::max(*mh, pitch_h);
    *mw = std::max(*mw, pitch_w);
    return MV_OK;
}

// An output (the buffers from `first_out` on) may overlap neither an input nor another output; empty buffers are not there.
struct Buffer {
    const char* name;
    const void* lo;
    size_t len;
};
int check_disjoint(const char* who, std::initializer_list<Buffer> buffers, size_t first_out) {
    const Buffer* v = buffers.begin();
    for (size_t o = first_out; o < buffers.size(); ++o)
        for (size_t i = 0; i < o; ++i) {
            const uintptr_t a = (uintptr_t)v[i].lo, b = (uintptr_t)v[o].lo;
            if (v[o].len && v[i].len && a < b + v[o].len && b < a + v[i].len) {
                set_error("%s: %s and %s overlap", who, v[i].name, v[o].name);
                return MV_E_UNSUPPORTED;
            }
        }
    return MV_OK;
}

// The host records of the boxes and the mix entry, in full: image inside x, box non-empty and inside its image, taps within the
// limit.  *mh, *mw: the most taps any box of the batch needs.
int check_boxes(const char* who, const mv_preprocess_box* rec_host, int B, int64_t x_bytes, int Hout, int Wout, int* mh, int* mw) {
    for (int i = 0; i < B; ++i) {
        const mv_preprocess_box& g = rec_host[i];
        if (const int rc = check_image(who, i, g.Hin, g.Win, true, g.offset, x_bytes)) return rc;
        MV_CHECK_ARG(g.h > 0 && g.w > 0 && g.top >= 0 && g.left >= 0 && (long long)g.top + g.h <= g.Hin &&
                         (long long)g.left + g.w <= g.Win,
                     "%s: image %d: box %dx%d at (%d, %d) does not lie inside the image %dx%d", who, i, g.h, g.w, g.top, g.left,
                     g.Hin, g.Win);
        if (const int rc = check_taps(who, i, "box ", g.h, g.w, Hout, Wout, nullptr, mh, mw)) return rc;
    }
    return MV_OK;
}

// The parameters every kernel takes; tab_h / tab_w stay NULL where the filter is generated, Hin / Win are the plain entry's alone
// (the record kernels fill them per image), the status word and the tile come from launch_tiles.
PrepP prep_params(const void* x, void* y, const float* a, const float* b, int Hout, int Wout, int mh, int mw) {
    PrepP p = {};
    p.x = (const uint8_t*)x; p.y = y; p.a = a; p.b = b;
    p.Hout = Hout; p.Wout = Wout; p.mh = mh; p.mw = mw;
    return p;
}

// One resize of a launch, per axis: input extent -> full output extent (before any crop or window).
struct Resize {
    int rows_in, rows_out, cols_in, cols_out;
};

// launches KERNEL<in_chw, out_nhwc, out_dtype == MV_BF16> with ARG on (grid, 256 threads, lds, st) of the calling entry
#define PREPROCESS_GO(KERNEL, ARG, CHW, NHWC, BF) hipLaunchKernelGGL((KERNEL<CHW, NHWC, BF>), grid, dim3(256), lds, st, ARG)
#define PREPROCESS_LAUNCH(KERNEL, ARG)                                                                                        \
    do {                                                                                                                      \
        const bool bf = out_dtype == MV_BF16;                                                                                 \
        if (in_chw) {                                                                                                         \
            if (out_nhwc) { if (bf) PREPROCESS_GO(KERNEL, ARG, true, true, true); else PREPROCESS_GO(KERNEL, ARG, true, true, false); }      \
            else { if (bf) PREPROCESS_GO(KERNEL, ARG, true, false, true); else PREPROCESS_GO(KERNEL, ARG, true, false, false); }             \
        } else {                                                                                                              \
            if (out_nhwc) { if (bf) PREPROCESS_GO(KERNEL, ARG, false, true, true); else PREPROCESS_GO(KERNEL, ARG, false, true, false); }    \
            else { if (bf) PREPROCESS_GO(KERNEL, ARG, false, false, true); else PREPROCESS_GO(KERNEL, ARG, false, false, false); }           \
        }                                                                                                                     \
    } while (0)

// The end of every entry.  One tile and one LDS size per launch: the staged rectangle is the largest any of the n resizes of the
// launch needs per axis (resize(i), i < n; p.mh / p.mw hold the largest pitches), so one steeply down-sampled image shrinks the
// tile -- and the occupancy -- of the whole launch.  Accepted: the result of an image does not depend on the tile it was computed
// in.  `what` names what did not fit; `keep`: see pick_tile.  The grid is tiles x tiles x B images, and for extra_elems > 0
// further z-slices behind the images whose workgroups stride over that many elements, about four per thread (the mix entry's
// targets).  The status word is fetched LAST: it is the first touch of the device, everything before it is host work.  Then
// launch(grid, lds, st), which is PREPROCESS_LAUNCH on the entry's kernel and parameters (p lives inside them).
template <class ResizeOf, class Launch>
int launch_tiles(const char* who, PrepP& p, int in_chw, int B, int n, ResizeOf&& resize, const char* what, bool keep, long long extra_elems,
                 mv_stream_t stream, Launch&& launch) {
    size_t lds = 0;
    if (!pick_tile(p, in_chw, &lds, [&](int TH, int TW, int* rows, int* cols) {
            *rows = *cols = 0;
            for (int i = 0; i < n; ++i) {
                const Resize g = resize(i);
                *rows = std::max(*rows, span_cap(TH, g.rows_in, g.rows_out));
                *cols = std::max(*cols, span_cap(TW, g.cols_in, g.cols_out));
            }
        }, keep)) {
        set_error("%s: %s does not fit the LDS tile (%zu bytes for the smallest tile)", who, what, lds);
        return MV_E_UNSUPPORTED;
    }
    const unsigned gx = (p.Wout + p.TW - 1) / p.TW, gy = (p.Hout + p.TH - 1) / p.TH;
    const long long per_slice = (long long)gx * gy * 256 * 4;
    const long long slices = extra_elems > 0 ? std::min<long long>((extra_elems + per_slice - 1) / per_slice, 65535 - B) : 0;
    const dim3 grid(gx, gy, B + (unsigned)slices);
    MV_CHECK_ARG(grid.y <= 65535, "%s: %d output rows are too many tiles", who, p.Hout);
    p.status = device_status_word();
    MV_CHECK_ARG(p.status != nullptr, "%s: the device status word is not available", who);
    set_kernel_name(who);
    launch(grid, lds, (hipStream_t)stream);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // namespace

}  // namespace mv

using namespace mv;

extern "C" {

int mv_preprocess_u8_fwd(const void* x, void* y, const void* tab_h, const void* tab_w, const float* a, const float* b, int B, int Hin,
                         int Win, int Hr, int Wr, int top, int left, int Hout, int Wout, int taps_h, int taps_w, int in_chw,
                         int out_dtype, int out_nhwc, mv_stream_t stream) {
    const char* who = "preprocess_u8";
    const int image[2] = {Hin, Win}, tables[2] = {taps_h, taps_w};
    if (const int rc = check_args(who, Hin > 0 && Win > 0 && Hr > 0 && Wr > 0 && Hout > 0 && Wout > 0 && taps_h > 0 && taps_w > 0, out_dtype,
                                  B, 65535, image))
        return rc;
    if (const int rc = check_buffers(who, {x, y, tab_h, tab_w, a, b})) return rc;
    if (top < 0 || left < 0 || (long long)top + Hout > Hr || (long long)left + Wout > Wr) {
        set_error("preprocess_u8: crop %dx%d at (%d, %d) does not lie inside the resized image %dx%d", Hout, Wout, top, left, Hr, Wr);
        return MV_E_UNSUPPORTED;
    }
    int mh = 0, mw = 0;
    if (const int rc = check_taps(who, -1, "", Hin, Win, Hr, Wr, tables, &mh, &mw)) return rc;
    if (const int rc = check_disjoint(who, {{"input", x, (size_t)B * Hin * Win * 3}, {"output", y, (size_t)B * 3 * Hout * Wout * dsize(out_dtype)}}, 1))
        return rc;

    PrepP p = prep_params(x, y, a, b, Hout, Wout, mh, mw);
    p.tab_h = (const int*)tab_h; p.tab_w = (const int*)tab_w; p.Hin = Hin; p.Win = Win;
    char what[64];
    snprintf(what, sizeof(what), "%dx%d -> %dx%d", Hin, Win, Hr, Wr);
    return launch_tiles(who, p, in_chw, B, 1, [&](int) { return Resize{Hin, Hr, Win, Wr}; }, what, false, 0, stream,
                        [&](dim3 grid, size_t lds, hipStream_t st) { PREPROCESS_LAUNCH(preprocess_u8_kernel, p); });
}

int mv_preprocess_u8_ragged_fwd(const void* x, int64_t x_bytes, void* y, const mv_preprocess_image* rec_host,
                                const mv_preprocess_image* rec_dev, const void* tab, int64_t tab_words, const float* a,
                                const float* b, int B, int Hout, int Wout, int in_chw, int out_dtype, int out_nhwc,
                                mv_stream_t stream) {
    const char* who = "preprocess_u8_ragged";
    if (const int rc = check_args(who, Hout > 0 && Wout > 0 && x_bytes > 0 && tab_words > 0, out_dtype, B, 65535)) return rc;
    if (const int rc = check_buffers(who, {x, y, rec_host, rec_dev, tab, a, b})) return rc;
    int mh = 0, mw = 0;
    for (int i = 0; i < B; ++i) {
        const mv_preprocess_image& g = rec_host[i];
        if (const int rc = check_image(who, i, g.Hin, g.Win, g.Hr > 0 && g.Wr > 0 && g.mh > 0 && g.mw > 0, g.offset, x_bytes)) return rc;
        if (g.top < 0 || g.left < 0 || (long long)g.top + Hout > g.Hr || (long long)g.left + Wout > g.Wr) {
            set_error("preprocess_u8_ragged: image %d: crop %dx%d at (%d, %d) does not lie inside the resized image %dx%d", i, Hout, Wout,
                      g.top, g.left, g.Hr, g.Wr);
            return MV_E_UNSUPPORTED;
        }
        const int tables[2] = {g.mh, g.mw};
        if (const int rc = check_taps(who, i, "", g.Hin, g.Win, g.Hr, g.Wr, tables, &mh, &mw)) return rc;
        MV_CHECK_ARG(g.tab_h >= 0 && g.tab_w >= 0 && (long long)g.tab_h + (long long)Hout * (2 + g.mh) <= tab_words &&
                         (long long)g.tab_w + (long long)Wout * (2 + g.mw) <= tab_words,
                     "preprocess_u8_ragged: image %d: tables at words %d and %d do not lie inside the table buffer of %lld words", i,
                     g.tab_h, g.tab_w, (long long)tab_words);
    }
    if (const int rc = check_disjoint(who, {{"input", x, (size_t)x_bytes}, {"output", y, (size_t)B * 3 * Hout * Wout * dsize(out_dtype)}}, 1))
        return rc;

    PrepRaggedP r;
    r.p = prep_params(x, y, a, b, Hout, Wout, mh, mw);
    r.p.tab_h = (const int*)tab;
    r.rec = rec_dev; r.x_bytes = x_bytes; r.tab_words = tab_words;
    return launch_tiles(who, r.p, in_chw, B, B, [&](int i) { return Resize{rec_host[i].Hin, rec_host[i].Hr, rec_host[i].Win, rec_host[i].Wr}; },
                        "the batch", false, 0, stream,
                        [&](dim3 grid, size_t lds, hipStream_t st) { PREPROCESS_LAUNCH(preprocess_u8_ragged_kernel, r); });
}

int mv_preprocess_u8_boxes_fwd(const void* x, int64_t x_bytes, void* y, const mv_preprocess_box* rec_host,
                               const mv_preprocess_box* rec_dev, const float* a, const float* b, int B, int Hout, int Wout,
                               int in_chw, int out_dtype, int out_nhwc, mv_stream_t stream) {
    const char* who = "preprocess_u8_boxes";
    if (const int rc = check_args(who, Hout > 0 && Wout > 0 && x_bytes > 0, out_dtype, B, 65535)) return rc;
    if (const int rc = check_buffers(who, {x, y, rec_host, rec_dev, a, b})) return rc;
    int mh = 0, mw = 0;
    if (const int rc = check_boxes(who, rec_host, B, x_bytes, Hout, Wout, &mh, &mw)) return rc;
    if (const int rc = check_disjoint(who, {{"input", x, (size_t)x_bytes}, {"output", y, (size_t)B * 3 * Hout * Wout * dsize(out_dtype)}}, 1))
        return rc;

    PrepBoxesP r;
    r.p = prep_params(x, y, a, b, Hout, Wout, mh, mw);
    r.rec = rec_dev; r.x_bytes = x_bytes;
    return launch_tiles(who, r.p, in_chw, B, B, [&](int i) { return Resize{rec_host[i].h, Hout, rec_host[i].w, Wout}; }, "the batch", false, 0,
                        stream, [&](dim3 grid, size_t lds, hipStream_t st) { PREPROCESS_LAUNCH(preprocess_u8_boxes_kernel, r); });
}

int mv_preprocess_u8_mix_fwd(const void* x, int64_t x_bytes, void* y, const mv_preprocess_box* rec_host,
                             const mv_preprocess_box* rec_dev, const mv_preprocess_mix* mix_host, const mv_preprocess_mix* mix_dev,
                             const float* a, const float* b, const int32_t* labels_host, const int32_t* labels_dev, float* targets,
                             int K, float on, float off, int B, int Hout, int Wout, int in_chw, int out_dtype, int out_nhwc,
                             mv_stream_t stream) {
    const char* who = "preprocess_u8_mix";
    if (const int rc = check_args(who, Hout > 0 && Wout > 0 && x_bytes > 0, out_dtype, B, 32767)) return rc;
    if (const int rc = check_buffers(who, {x, y, rec_host, rec_dev, mix_host, mix_dev, a, b})) return rc;
    MV_CHECK_ARG((labels_dev != nullptr) == (targets != nullptr), "preprocess_u8_mix: labels and targets go together, got %s without %s",
                 labels_dev ? "labels" : "targets", labels_dev ? "targets" : "labels");
    MV_CHECK_ARG(!labels_host || labels_dev, "preprocess_u8_mix: a host copy of the labels without the device labels");
    MV_CHECK_ARG(!labels_dev || (K > 0 && (long long)B * K < (1LL << 31)), "preprocess_u8_mix: %d classes for %d images", K, B);
    int mh = 0, mw = 0;
    if (const int rc = check_boxes(who, rec_host, B, x_bytes, Hout, Wout, &mh, &mw)) return rc;
    auto unit = [](float v) { return std::isfinite(v) && v >= 0.f && v <= 1.f; };
    auto inside = [&](int y0, int x0, int y1, int x1) {
        return y0 >= 0 && y0 <= Hout && y1 >= 0 && y1 <= Hout && x0 >= 0 && x0 <= Wout && x1 >= 0 && x1 <= Wout;
    };
    bool keep = false;
    for (int i = 0; i < B; ++i) {
        const mv_preprocess_mix& m = mix_host[i];
        MV_CHECK_ARG(m.partner >= 0 && m.partner < B, "preprocess_u8_mix: image %d: partner %d does not lie in [0, %d)", i, m.partner, B);
        MV_CHECK_ARG(unit(m.lam) && unit(m.oml) && unit(m.lam_t) && unit(m.oml_t),
                     "preprocess_u8_mix: image %d: lam %g, oml %g, lam_t %g, oml_t %g must be finite and lie in [0, 1]", i,
                     (double)m.lam, (double)m.oml, (double)m.lam_t, (double)m.oml_t);
        MV_CHECK_ARG(inside(m.cy0, m.cx0, m.cy1, m.cx1),
                     "preprocess_u8_mix: image %d: cut rectangle (%d, %d, %d, %d) does not lie inside the output %dx%d", i, m.cy0, m.cx0,
                     m.cy1, m.cx1, Hout, Wout);
        MV_CHECK_ARG(inside(m.ey0, m.ex0, m.ey1, m.ex1),
                     "preprocess_u8_mix: image %d: erase rectangle (%d, %d, %d, %d) does not lie inside the output %dx%d", i, m.ey0,
                     m.ex0, m.ey1, m.ex1, Hout, Wout);
        MV_CHECK_ARG(!labels_host || (labels_host[i] >= 0 && labels_host[i] < K),
                     "preprocess_u8_mix: image %d: label %d does not lie in [0, %d)", i, labels_host ? labels_host[i] : 0, K);
        keep |= m.partner != i;
    }
    if (const int rc = check_disjoint(who, {{"images", x, (size_t)x_bytes}, {"output", y, (size_t)B * 3 * Hout * Wout * dsize(out_dtype)},
                                            {"targets", targets, targets ? (size_t)B * K * 4 : 0}}, 1))
        return rc;

    // with a partner anywhere in the batch the tile also keeps the partner's results (TH x 3 x TW fp32) while its own window is staged
    PrepMixP r;
    r.p = prep_params(x, y, a, b, Hout, Wout, mh, mw);
    r.rec = rec_dev; r.mix = mix_dev; r.x_bytes = x_bytes; r.labels = labels_dev; r.targets = targets;
    r.B = B; r.K = K; r.keep = keep; r.on = on; r.off = off;
    return launch_tiles(who, r.p, in_chw, B, B, [&](int i) { return Resize{rec_host[i].h, Hout, rec_host[i].w, Wout}; }, "the batch", keep,
                        targets ? (long long)B * K : 0, stream,
                        [&](dim3 grid, size_t lds, hipStream_t st) { PREPROCESS_LAUNCH(preprocess_u8_mix_kernel, r); });
}

int mv_preprocess_u8_seg_fwd(const void* x, int64_t x_bytes, const void* m, int64_t m_bytes, void* y, int32_t* labels,
                             const mv_preprocess_seg* rec_host, const mv_preprocess_seg* rec_dev, const float* a, const float* b,
                             int B, int Hout, int Wout, int image_fill, int mask_fill, int in_chw, int out_dtype, int out_nhwc,
                             mv_stream_t stream) {
    const char* who = "preprocess_u8_seg";
    if (const int rc = check_args(who, Hout > 0 && Wout > 0 && x_bytes > 0, out_dtype, B, 65535)) return rc;
    MV_CHECK_ARG((m != nullptr) == (labels != nullptr), "preprocess_u8_seg: masks and labels go together, got %s without %s",
                 m ? "masks" : "labels", m ? "labels" : "masks");
    MV_CHECK_ARG(!m || m_bytes > 0, "preprocess_u8_seg: bad sizes");
    MV_CHECK_ARG(image_fill >= 0 && image_fill <= 255 && mask_fill >= 0 && mask_fill <= 255,
                 "preprocess_u8_seg: image_fill %d and mask_fill %d must lie in [0, 255]", image_fill, mask_fill);
    if (const int rc = check_buffers(who, {x, y, rec_host, rec_dev, a, b})) return rc;
    int mh = 0, mw = 0;
    for (int i = 0; i < B; ++i) {
        const mv_preprocess_seg& g = rec_host[i];
        if (const int rc = check_image(who, i, g.Hin, g.Win, g.Hr > 0 && g.Wr > 0, g.offset, x_bytes)) return rc;
        const long long px = (long long)g.Hin * g.Win;
        MV_CHECK_ARG(!m || (g.mask_offset >= 0 && g.mask_offset <= m_bytes - px),
                     "preprocess_u8_seg: image %d: mask of %lld bytes at offset %lld does not lie inside the buffer of %lld bytes", i, px,
                     (long long)g.mask_offset, (long long)m_bytes);
        const int Hp = std::max(g.Hr, Hout), Wp = std::max(g.Wr, Wout);
        MV_CHECK_ARG(g.top >= 0 && g.left >= 0 && (long long)g.top + Hout <= Hp && (long long)g.left + Wout <= Wp,
                     "preprocess_u8_seg: image %d: window %dx%d at (%d, %d) does not lie inside the padded image %dx%d", i, Hout, Wout,
                     g.top, g.left, Hp, Wp);
        if (const int rc = check_taps(who, i, "", g.Hin, g.Win, g.Hr, g.Wr, nullptr, &mh, &mw)) return rc;
    }
    const size_t px_out = (size_t)B * Hout * Wout;       // x and m are only read
    if (const int rc = check_disjoint(who, {{"images", x, (size_t)x_bytes}, {"masks", m, m ? (size_t)m_bytes : 0},
                                            {"output", y, px_out * 3 * dsize(out_dtype)}, {"labels", labels, labels ? px_out * 4 : 0}}, 2))
        return rc;

    PrepSegP r;
    r.p = prep_params(x, y, a, b, Hout, Wout, mh, mw);
    r.rec = rec_dev; r.m = (const uint8_t*)m; r.labels = labels; r.x_bytes = x_bytes; r.m_bytes = m ? m_bytes : 0;
    r.image_fill = image_fill; r.mask_fill = mask_fill;
    return launch_tiles(who, r.p, in_chw, B, B, [&](int i) { return Resize{rec_host[i].Hin, rec_host[i].Hr, rec_host[i].Win, rec_host[i].Wr}; },
                        "the batch", false, 0, stream,
                        [&](dim3 grid, size_t lds, hipStream_t st) { PREPROCESS_LAUNCH(preprocess_u8_seg_kernel, r); });
}

}  // extern "C"
