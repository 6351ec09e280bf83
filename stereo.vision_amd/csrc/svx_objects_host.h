// Host-only part of the obstacle list's runtime (rt_objects.hip): the argument checks of sv_obstacle_list and the
// size of the labelling scratch. No HIP in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svx.h"

namespace svx {

constexpr int kObjMaxCap = 32;           // entries of a frame's list (a 256-bin histogram each: 32 KB of LDS)
constexpr int kObjMaxSlots = 1024;       // workgroups of a launch, each with a scratch slot of its own
constexpr size_t kObjScratchBudget = (size_t)2 << 30;   // bytes of labelling scratch a launch may hold

// nullptr when sv_obstacle_list's arguments are in range, else what is wrong with them
inline const char* objects_check_args(const void* obstacles, int H, int W, int min_area, const void* out, int cap,
                                      const void* n) {
    if (!obstacles || !out || !n) return "null obstacle image, list or count";
    if (H < 1 || H > 4096) return "1 <= H <= 4096";
    if (W < 2 || W > 4096) return "2 <= W <= 4096";
    if (min_area < 1) return "min_area >= 1";
    if (cap < 1 || cap > kObjMaxCap) return "1 <= cap <= 32";
    return nullptr;
}

// The labelling scratch. A bitmap word holds at most 16 run starts and two of them never share an even / odd pixel
// pair, so a row has 16 WW node slots (WW = ceil(W / 32)) and a frame H x 16 WW. A workgroup owns one scratch slot:
// a parent table and an area table of int32, 128 H WW bytes together (2.2 MB for 544 x 1024, 128 MB for 4096 x
// 4096), and takes frame after frame through it. The launch has as many workgroups as the budget holds slots, at
// most kObjMaxSlots and at most one a frame, so the scratch depends on the shape alone: never on the number of
// frames past that, never on what the bitmaps hold.
struct ObjLayout {
    int WW = 0, HW = 0;        // words a bitmap row; node slots a row
    size_t nodes = 0;          // node slots a frame (entries of each table)
    int slots = 0;             // workgroups of the launch
    size_t off_area = 0, bytes = 0;   // the parent tables at 0, the area tables behind them
};

inline ObjLayout objects_layout(int H, int W, int frames) {
    ObjLayout l;
    l.WW = (W + 31) / 32;
    l.HW = 16 * l.WW;
    l.nodes = (size_t)H * (size_t)l.HW;
    const size_t per_slot = 2 * sizeof(int32_t) * l.nodes;
    size_t slots = kObjScratchBudget / per_slot;
    if (slots > (size_t)kObjMaxSlots) slots = kObjMaxSlots;
    if (slots > (size_t)frames) slots = frames > 0 ? (size_t)frames : 1;
    if (slots < 1) slots = 1;
    l.slots = (int)slots;
    l.off_area = sizeof(int32_t) * l.nodes * slots;
    l.bytes = 2 * l.off_area;
    return l;
}

}  // namespace svx
