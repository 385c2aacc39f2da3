// atr_view_rule.h — the player views' arithmetic (include/atr_view.h), plain C++17 with no HIP dependence: the kernels
// (view_hip.hip k_view_cells, k_view_rgb) and the host test program (tests/view_host.cpp) both use it. The un-turn of an
// egocentric window is atr_ego::src_cell (atr_ego_rule.h), which is not restated here.
//
// A code is band * 16 + value. Band 0: what the viewer was shown (a known window value, or 15). Band 1: the truth under a cell
// the viewer's window shows as hidden (5). Band 2: the truth outside the viewer's window. 255: outside the env's own map.
#pragma once

#include "atr_ego_rule.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATR_VIEW_HD __host__ __device__ constexpr
#else
#define ATR_VIEW_HD constexpr
#endif

namespace atr_view {

constexpr int kSide = 82, kWin = 13, kPob = 6, kWindow = kWin * kWin;
constexpr int kUnknown = 15, kHidden = 5, kOutside = 255, kBandHidden = 16, kBandBeyond = 32;
// the canvas, in cells: the map panel, a gap, the tracker's window at kZoom canvas cells per window cell, a gap, the target's
constexpr int kCanvasH = 82, kCanvasW = 242, kGap = 2, kZoom = 6;
constexpr int kWinRows = kWin * kZoom, kWin0X0 = kSide + kGap, kWin1X0 = kWin0X0 + kWinRows + kGap;   // 78, 84, 164
static_assert(kWin1X0 + kWinRows == kCanvasW && kCanvasH == kSide, "the three panels fill the canvas");

// colours, r | g << 8 | b << 16
constexpr unsigned kRgbFree = 0xffffffu, kRgbWall = 0x000000u, kRgbTracker = 0xff0000u, kRgbTarget = 0x0000ffu,
                   kRgbPrint = 0x00ffffu, kRgbUnseen = 0x505050u, kRgbMemWall = 0x303060u, kRgbMemFree = 0xc0c0e8u,
                   kRgbUnknown = 0xff00ffu, kRgbBackground = 0x808080u;

// A window value as a code: itself when it is one of 0, 1, 2, 4, 5, 6, 7, 8, else kUnknown.
ATR_VIEW_HD int known(int v) { return v >= 0 && v <= 8 && v != 3 ? v : kUnknown; }
// ... of a float window: the value must equal the integer exactly (a NaN equals nothing)
ATR_VIEW_HD int known(float v)
{
    return v == 0.0f ? 0 : v == 1.0f ? 1 : v == 2.0f ? 2 : v == 4.0f ? 4 : v == 5.0f ? 5 : v == 6.0f ? 6 : v == 7.0f ? 7
         : v == 8.0f ? 8 : kUnknown;
}

// The truth on a map cell: the map bit, then 2 on the tracker's cell, then 4 on the target's.
ATR_VIEW_HD int truth(int map_bit, bool tracker_here, bool target_here) { return target_here ? 4 : tracker_here ? 2 : map_bit; }

// Where cell `cell` of the window as given goes in the viewer's absolute window.
ATR_VIEW_HD int unturn_cell(bool turned, int heading, int cell) { return turned ? atr_ego::src_cell(heading, cell) : cell; }

// Is the offset (dr, dc) from the viewer inside its window?
ATR_VIEW_HD bool in_window(int dr, int dc) { return dr >= -kPob && dr <= kPob && dc >= -kPob && dc <= kPob; }
ATR_VIEW_HD int window_index(int dr, int dc) { return (kPob + dr) * kWin + kPob + dc; }

// The map panel's code of a cell inside the env's map: truth t, and (when inside the window) the absolute window's code w there.
ATR_VIEW_HD int map_code(int t, bool inside, int w) { return !inside ? kBandBeyond + t : w == kHidden ? kBandHidden + t : w; }

// The colour of a window value (band 0 and the window panels).
ATR_VIEW_HD unsigned value_rgb(int v)
{
    return v == 0 ? kRgbFree : v == 1 ? kRgbWall : v == 2 ? kRgbTracker : v == 4 ? kRgbTarget : v == 5 ? kRgbUnseen
         : v == 6 ? kRgbPrint : v == 7 ? kRgbMemWall : v == 8 ? kRgbMemFree : v == kUnknown ? kRgbUnknown : kRgbBackground;
}

ATR_VIEW_HD unsigned dim_rgb(unsigned rgb, int add, int shift)
{
    return (((rgb & 0xffu) + (unsigned)add) >> shift) | (((((rgb >> 8) & 0xffu) + (unsigned)add) >> shift) << 8)
         | (((((rgb >> 16) & 0xffu) + (unsigned)add) >> shift) << 16);
}

// The colour of a code. Bands 1 and 2 carry a truth (0, 1, 2 or 4); everything that is no code is the background.
ATR_VIEW_HD unsigned code_rgb(int code)
{
    const int band = code >> 4, v = code & 15;
    const bool is_truth = v == 0 || v == 1 || v == 2 || v == 4;
    return band == 0 ? value_rgb(v) : band == 1 && is_truth ? dim_rgb(value_rgb(v), 128, 1)
         : band == 2 && is_truth ? dim_rgb(value_rgb(v), 384, 2) : kRgbBackground;
}

} // namespace atr_view
