// build_launch.h -- what the device BVH builder's kernels (kernels/build.hip) and their host driver (bvh_device.cpp) share.
#pragma once
#include <hip/hip_runtime.h>

#include "../bvh.h"
#include "../bvh_level.h"

namespace pyr {
namespace devbuild {

// A node of more than kSmallNode references is binned and partitioned by many workgroups, kChunk references each, through
// global atomics; one of at most kSmallNode -- a wave's worth -- by one wave, from bins to children, without any.
constexpr uint32_t kSmallNode = kLevelSmallNode;
constexpr uint32_t kChunk = kLevelChunk;
constexpr uint32_t kBlock = 256;
// the largest node one workgroup splits by the median rule (its keys live in LDS: 8 bytes each); a larger one ends the device build
constexpr uint32_t kMedianMax = 2048;
constexpr uint32_t kBinWords = 3 * lvl::kBins * 7; // per node: lower keys [axis][bin][3], upper keys [axis][bin][3], counts [axis][bin]

enum : uint32_t { GIVEUP_NONE = 0, GIVEUP_MEDIAN_TOO_LARGE = 1, GIVEUP_CAPACITY = 2 };

struct Chunk {
    uint32_t task, large_index, begin, end;
};

struct Counters {
    uint32_t num_tasks;
    uint32_t num_large[2], num_small[2], num_chunks[2]; // [level parity]
    uint32_t giveup;
};

struct Ctx {
    lvl::Task* tasks;
    PrimBounds* refs[2]; // [level parity]: a level reads its own and writes the next one's
    uint32_t* leaf_shapes;
    uint32_t* bins;
    uint32_t* large_list[2];
    uint32_t* small_list[2];
    Chunk* chunks[2];
    Counters* counters;
    uint32_t n, max_tasks, max_large, max_small, max_chunks;
    uint32_t in_pairs, depth_bound;
};

// Each enqueues on `stream` and returns hipGetLastError(). `parity`: the level's (level & 1).
hipError_t launch_setup(const Ctx& c, hipStream_t stream);                       // task 0 = the whole range with its bounds, level 0's lists
hipError_t launch_level(const Ctx& c, uint32_t parity, uint32_t num_large, uint32_t num_small, uint32_t num_chunks, hipStream_t stream);

} // namespace devbuild
} // namespace pyr
