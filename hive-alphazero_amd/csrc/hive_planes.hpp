// hive_planes.hpp -- the store half of the plane writer, shared by hive_expand_kernel (hive_env.hip) and the replay
// sampler (hive_replay.hip): a board's 144 completed 56-bit cell words in LDS -> its 8,064 plane elements in HBM.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/hive_abi.h"
#include "hive_bb.hpp"
#include "hive_tables.hpp"

namespace hive {

// value encoders for the plane writer
template <typename T> struct PlaneVal;
template <> struct PlaneVal<float> {
    static __device__ __forceinline__ uint32_t one() { return 0x3F800000u; }
    static __device__ __forceinline__ uint32_t of(unsigned v) { return __float_as_uint((float)v); }
};
struct half_tag {};
struct bf16_tag {};
template <> struct PlaneVal<half_tag> {
    static __device__ __forceinline__ uint32_t one() { return 0x3C00u; }
    static __device__ __forceinline__ uint32_t of(unsigned v)
    {
        _Float16 hval = (_Float16)(float)v;
        return (uint32_t) __builtin_bit_cast(unsigned short, hval);
    }
};
template <> struct PlaneVal<bf16_tag> {
    static __device__ __forceinline__ uint32_t one() { return 0x3F80u; }
    static __device__ __forceinline__ uint32_t of(unsigned v) { return __float_as_uint((float)v) >> 16; }   // v <= 255: exact
};
template <int DT>
using PlaneType = typename std::conditional<DT == 0, float, typename std::conditional<DT == 1, half_tag, bf16_tag>::type>::type;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// NT: streaming (nontemporal) stores for launches whose output is far larger than the caches -- 5.3 instead of 4.2 TB/s at
// 65,536 boards (1 GB of planes); leaf batches of a search (<= 4096 boards, read back at once by the network) keep plain stores
template <bool NT>
__device__ __forceinline__ void plane_store(u32x4 val, u32x4 *ptr)
{
    if (NT) __builtin_nontemporal_store(val, ptr);
    else *ptr = val;
}
constexpr int kExpandStreamBoards = 8192;              // from this many boards per launch (127 MB of bf16 planes) on: NT stores
constexpr int kExpandAhead = 4;                        // boards whose inputs are in flight per workgroup
constexpr long long kExpandMaxBlocks = 256 * 8;       // all resident at once: 8 workgroups of 4 waves per CU
constexpr int kPlaneItems = kCells * HIVE_PLANES / 8;  // 1008 items of 8 elements per board = 4 x 252

// A 256-thread workgroup writes board `b` of `planes` from the completed cell words `full[144]` (LDS): thread t writes the
// 16-byte (f16 / bf16; 32-byte f32) items t, t + 256, t + 512, t + 768 (< 1008): every wave's store is one
// 128-byte-aligned KiB.  `one` = PlaneVal::one(), `tv` = PlaneVal::of(turn) (plane 31 = raw turn number, env_hive.py:331).
template <int DT, int LAYOUT, bool NT>
__device__ __forceinline__ void plane_store_board(const unsigned long long *full, uint32_t one, uint32_t tv, void *planes,
                                                  long long b, int tid)
{
    HIVE_UNROLL for (int j = 0; j < 4; ++j) {
        if (j == 3 && tid >= kPlaneItems - 768) break;
        const int e0 = (tid + j * 256) * 8;
        uint32_t v[8];
        if (LAYOUT == HIVE_HWC) {
            const int cell = e0 / HIVE_PLANES, p0 = e0 - cell * HIVE_PLANES;
            const unsigned bits8 = (unsigned)(full[cell] >> p0) & 0xFFu;
            HIVE_UNROLL for (int k = 0; k < 8; ++k) v[k] = ((bits8 >> k) & 1u) ? one : 0u;
            if (p0 == 24) v[7] = tv;      // plane 31 = raw turn number (env_hive.py:331)
        } else {
            const int pl = e0 / kCells, c0 = e0 - pl * kCells;
            HIVE_UNROLL for (int k = 0; k < 8; ++k) v[k] = ((full[c0 + k] >> pl) & 1ull) ? one : 0u;
            if (pl == 31) { HIVE_UNROLL for (int k = 0; k < 8; ++k) v[k] = tv; }
        }
        const long long eoff = b * (long long)(kCells * HIVE_PLANES) + e0;
        if (DT == 0) {
            u32x4 *dst = reinterpret_cast<u32x4 *>(reinterpret_cast<float *>(planes) + eoff);
            plane_store<NT>(u32x4{v[0], v[1], v[2], v[3]}, dst);
            plane_store<NT>(u32x4{v[4], v[5], v[6], v[7]}, dst + 1);
        } else {
            u32x4 *dst = reinterpret_cast<u32x4 *>(reinterpret_cast<uint16_t *>(planes) + eoff);
            plane_store<NT>(u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)}, dst);
        }
    }
}

}  // namespace hive
