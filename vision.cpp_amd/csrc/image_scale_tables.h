// The table block of vx_image_scale: what image_scale_device.cpp packs and kernels_imgscale.hip reads, laid out by one function so that the
// two cannot disagree. Plain C++ without HIP or host-library types; every offset is in 32-bit words from the start of the block.
//
//   lut      [640]                  sRGB -> linear [256] f32, alpha v / 255.0f [256] f32, the sRGB encoder's pairs [104] u32, padding
//   xfirst   [ow], xcount [ow]      per output column: first source column of its taps (unclamped, may be negative) and their number
//   tile_xlo [tiles_x], tile_span   per tile of tile_w columns: the lowest xfirst and the number of (unclamped) source columns its taps reach
//   xw       [tiles_x][taps_x][tile_w]  the weights, tap-major inside a tile: the lanes of a wave read consecutive words
//   yfirst   [oh], ycount [oh]      the same per output row
//   band_lo  [tiles_y], band_n      per tile of TH rows: the first (unclamped) source row of its band and the band's length
//   yw       [oh][taps_y]           the vertical weights, row-major
#pragma once
#include <cstddef>

namespace visp_scale {

constexpr int TW = 64;                 // output columns of a tile: with the channel as the fast thread index a block is 64 x ch threads (1, 3 or 4 waves)
constexpr int TH = 8;                  // output rows of a tile = vertical accumulators a thread keeps in registers
constexpr int MAX_TAPS = 768;          // per output sample and axis; at tile_w 1 and 4 channels the tables of 768 x 768 taps take 54.7 KB of LDS
constexpr int LDS_BUDGET = 64 * 1024;  // what a launch may ask for without raising the kernel's dynamic-LDS attribute
constexpr int LUT_WORDS = 640;

struct table_layout {
    int tiles_x, tiles_y;
    size_t xfirst, xcount, tile_xlo, tile_span, xw, yfirst, ycount, band_lo, band_n, yw, total;
};

inline table_layout layout(int ow, int oh, int tile_w, int taps_x, int taps_y) {
    table_layout l{};
    l.tiles_x = (ow + tile_w - 1) / tile_w;
    l.tiles_y = (oh + TH - 1) / TH;
    size_t at = LUT_WORDS;
    auto take = [&at](size_t n) { const size_t o = at; at += n; return o; };
    l.xfirst = take((size_t)ow);
    l.xcount = take((size_t)ow);
    l.tile_xlo = take((size_t)l.tiles_x);
    l.tile_span = take((size_t)l.tiles_x);
    l.xw = take((size_t)l.tiles_x * taps_x * tile_w);
    l.yfirst = take((size_t)oh);
    l.ycount = take((size_t)oh);
    l.band_lo = take((size_t)l.tiles_y);
    l.band_n = take((size_t)l.tiles_y);
    l.yw = take((size_t)oh * taps_y);
    l.total = at;
    return l;
}

// LDS words of a block, in the kernel's order: the lookup tables (u8 formats), yfirst / ycount of the tile's rows, their weights, the tile's
// horizontal weights, the alpha of every output of the tile (the un-premultiply reads a neighbour thread's accumulator) and two row buffers
constexpr size_t lds_words(int ch, bool f32, int tile_w, int taps_x, int taps_y, int span) {
    return (f32 ? 0 : (size_t)LUT_WORDS) + 2 * TH + (size_t)TH * taps_y + (size_t)taps_x * tile_w + (size_t)TH * tile_w + 2 * (size_t)span * ch;
}
static_assert(lds_words(4, false, 1, MAX_TAPS, MAX_TAPS, MAX_TAPS) * 4 <= LDS_BUDGET, "the tap limit must fit a one-column tile");

} // namespace visp_scale
