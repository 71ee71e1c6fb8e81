// hive_replay.hip -- the replay window on the GPU: the most recent `capacity` self-play rows kept as the engine emits them
// (packed features, history words, sparse visit policy: ~2.9 KB per slot instead of 38.6 KB of dense fp32) and the fused
// "draw, gather, widen, scatter" kernel that turns sampled rows into the trainer's tensors in one launch.
//
// AlphaZero trains on a sliding window of the most recent games (the reference's woker/optimize.py loads the recent
// play_*.json files); here the window is a ring of row slots in HBM, structure-of-arrays:
//
//   feat  u64[capacity][144]      the packed 56-bit cell words (planes 31 and 36..43 are not part of them)
//   hist  u32[capacity][4][2][6]  the MOVER's history bitboards (age, own / enemy, word)
//   meta  u32[capacity]           bytes: valid history entries, turn, mover, 0
//   value f32[capacity]           the training value (records.packed_values: result from the mover's side, discounted)
//   cnt   i32[capacity]           entries of the visit policy (<= HIVE_LIST_CAP: a position has no more edges)
//   idx   i16[capacity][256], val f32[capacity][256]   the policy's columns and weights; the tail is zero
//
//   replay_write_kernel   one workgroup per appended row: copies the row into slot (head + i) mod capacity, turns the CSR
//                         policy into the fixed-width form and computes the value from the row's whole game
//   replay_sample_kernel  one workgroup per sampled row: completes the 144 cell words in LDS (history planes 36..43 with the
//                         plane writer's perspective / valid-entry rule), stores the planes with the writer's item pattern
//                         (plane_store_board, hive_planes.hpp), builds the dense policy row in LDS and stores it as whole
//                         16-byte pieces, writes the value
//   replay_export_kernel  the live rows in logical order (checkpoints, tests)
//
// The write position and the live count live on the host (appends are host-driven): nothing but stats / export waits for
// the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/hive_abi.h"
#include "hive_planes.hpp"
#include "hive_rng.hpp"

namespace hive {
int set_error(int code, const std::string &msg);
}

struct HiveReplay {
    int device = 0;
    long long capacity = 0;
    long long head = 0;                       // slot the next appended row goes to
    long long live = 0;                       // rows in the window (the oldest sits in slot (head - live) mod capacity)
    long long appended = 0;                   // rows ever appended
    unsigned long long *feat = nullptr;       // [capacity][144]
    uint32_t *hist = nullptr;                 // [capacity][48]
    uint32_t *meta = nullptr;                 // [capacity]
    float *value = nullptr;                   // [capacity]
    int32_t *cnt = nullptr;                   // [capacity]
    int16_t *idx = nullptr;                   // [capacity][256]
    float *val = nullptr;                     // [capacity][256]
    float *discount = nullptr;                // [256]
};

namespace {
using namespace hive;

constexpr int kHistWords = 48;                            // u32[4][2][6]
constexpr int kPolPieces = HIVE_ACTIONS * 4 / 16;         // 396 16-byte pieces of a dense policy row
constexpr long long kReplayMaxBlocks = kExpandMaxBlocks;  // the planes writer's grid-stride cap
static_assert(HIVE_ACTIONS * 4 % 16 == 0, "a policy row is a whole number of 16-byte pieces");

#define REPLAY_TRY(expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return hive::set_error(HIVE_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

struct Ring {
    unsigned long long *feat;
    uint32_t *hist, *meta;
    float *value;
    int32_t *cnt;
    int16_t *idx;
    float *val;
    long long capacity;
};

// Batch rows skip .. rows - 1 -> slots (head + row) mod capacity.  PACKED: the batch is in the .npz layout (CSR policies,
// values from game_ptr / game_val); otherwise in the export layout (fixed-width policies, values as given).
template <bool PACKED>
__global__ void __launch_bounds__(256)
replay_write_kernel(Ring ring, long long head, long long skip, long long rows, long long games,
                    const unsigned long long *__restrict__ feat, const uint32_t *__restrict__ hist, const uint8_t *__restrict__ meta,
                    const int16_t *__restrict__ pol_idx, const float *__restrict__ pol_val, const long long *__restrict__ pol_ptr,
                    const int32_t *__restrict__ pol_cnt, const long long *__restrict__ game_ptr, const int8_t *__restrict__ game_val,
                    const float *__restrict__ values, const float *__restrict__ discount, const long long *__restrict__ rank,
                    long long rank_skip)
{
    __shared__ int later;                                  // later moves of the row's side in its game
    const int tid = threadIdx.x;
    for (long long i = skip + blockIdx.x; i < rows; i += gridDim.x) {
        // rank (hive_replay_append_ranked): the row's place among the rows that are kept, -1 = not a row of the window; of more
        // kept rows than the ring holds the first rank_skip are left out (the same for the whole workgroup).  The rows of its
        // game below are walked whether they are kept or not
        const long long dest = rank != nullptr ? rank[i] : i;
        if (dest < rank_skip) continue;
        const size_t slot = (size_t)((head + dest) % ring.capacity);
        if (tid < kCells) ring.feat[slot * kCells + tid] = feat[i * kCells + tid];
        else if (tid < kCells + kHistWords) ring.hist[slot * kHistWords + (tid - kCells)] = hist[i * kHistWords + (tid - kCells)];
        const int stride = PACKED ? 3 : 4;
        const unsigned mover = meta[i * stride + 2];
        if (tid == 255)
            ring.meta[slot] = (uint32_t)meta[i * stride] | ((uint32_t)meta[i * stride + 1] << 8) | ((uint32_t)mover << 16);
        long long p0 = (long long)i * HIVE_LIST_CAP, pc = 0;
        if (PACKED) {
            p0 = pol_ptr[i];
            pc = pol_ptr[i + 1] - p0;
        } else {
            pc = pol_cnt[i];
        }
        const int c = (int)(pc < 0 ? 0 : pc > HIVE_LIST_CAP ? HIVE_LIST_CAP : pc);
        ring.idx[slot * HIVE_LIST_CAP + tid] = tid < c ? pol_idx[p0 + tid] : (int16_t)0;
        ring.val[slot * HIVE_LIST_CAP + tid] = tid < c ? pol_val[p0 + tid] : 0.0f;
        if (tid == 0) ring.cnt[slot] = c;
        if (!PACKED) {
            if (tid == 0) ring.value[slot] = values[i];
            continue;
        }
        // the row's game: the last g with game_ptr[g] <= i (empty games repeat a pointer)
        long long lo = 0, hi = games;                      // game_ptr[lo] <= i < game_ptr[hi]
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (game_ptr[mid] <= i) lo = mid; else hi = mid;
        }
        const long long gend = game_ptr[lo + 1] < rows ? game_ptr[lo + 1] : rows;
        if (tid == 0) later = 0;
        __syncthreads();
        int mine = 0;
        for (long long r = i + 1 + tid; r < gend; r += 256) mine += meta[r * 3 + 2] == mover ? 1 : 0;
        if (mine) atomicAdd(&later, mine);
        __syncthreads();
        if (tid == 0) {
            const int vw = game_val[lo];
            const float v = vw == 0 ? -1.0f : (float)(mover == 0u ? vw : -vw);
            const int k = later > 255 ? 255 : later;
            ring.value[slot] = k > 0 ? v * discount[k] : v;
        }
    }
}

__global__ void __launch_bounds__(256)
replay_export_kernel(Ring ring, long long oldest, long long live, unsigned long long *__restrict__ feat, uint32_t *__restrict__ hist,
                     uint8_t *__restrict__ meta, int32_t *__restrict__ pol_cnt, int16_t *__restrict__ pol_idx,
                     float *__restrict__ pol_val, float *__restrict__ values)
{
    const int tid = threadIdx.x;
    for (long long i = blockIdx.x; i < live; i += gridDim.x) {
        const size_t slot = (size_t)((oldest + i) % ring.capacity);
        if (feat && tid < kCells) feat[i * kCells + tid] = ring.feat[slot * kCells + tid];
        if (hist && tid >= kCells && tid < kCells + kHistWords)
            hist[i * kHistWords + (tid - kCells)] = ring.hist[slot * kHistWords + (tid - kCells)];
        if (meta && tid >= 252) meta[i * 4 + (tid - 252)] = (uint8_t)(ring.meta[slot] >> (8 * (tid - 252)));
        if (pol_idx) pol_idx[i * HIVE_LIST_CAP + tid] = ring.idx[slot * HIVE_LIST_CAP + tid];
        if (pol_val) pol_val[i * HIVE_LIST_CAP + tid] = ring.val[slot * HIVE_LIST_CAP + tid];
        if (tid == 0) {
            if (pol_cnt) pol_cnt[i] = ring.cnt[slot];
            if (values) values[i] = ring.value[slot];
        }
    }
}

// entry i of a device-drawn minibatch: a pure function of (seed, step, stream_id, i, live); the high half of a 32 x 32 bit
// product is free of modulo bias beyond 2^-32 (replay.draw_indices is the Python mirror)
__device__ __forceinline__ long long replay_draw(unsigned long long seed, unsigned long long step, unsigned long long stream_id,
                                                 unsigned long long i, unsigned long long live)
{
    Rng g(seed, step, stream_id, i);
    const unsigned long long x = splitmix(g.s);
    return (long long)(((x >> 32) * live) >> 32);
}

// One workgroup per sampled row (grid-stride).  Two LDS images per row, both double-buffered so that a fast wave may start
// the next row while a slow one still reads this one: the 144 completed cell words and the dense policy row (6,336 B).
// The policy row is zeroed and scattered in LDS -- zeroing it in global memory and scattering into it from other threads
// would need the zero stores acknowledged first -- which takes a barrier between the zero fill and the scatter and one
// before the stores; both wait for LDS only, never for the previous row's global stores.
template <int DT, int LAYOUT, bool NT>
__global__ void __launch_bounds__(256)
replay_sample_kernel(Ring ring, long long oldest, long long live, const long long *__restrict__ indices, unsigned long long seed,
                     unsigned long long step, unsigned long long stream_id, int n, void *__restrict__ planes,
                     float *__restrict__ policies, float *__restrict__ values, long long *__restrict__ indices_out)
{
    using V = PlaneType<DT>;
    __shared__ unsigned long long full[2][kCells];
    __shared__ __attribute__((aligned(16))) float pol[2][HIVE_ACTIONS];
    const uint32_t one = PlaneVal<V>::one();
    const int tid = threadIdx.x;
    int buf = 0;
    for (long long o = blockIdx.x; o < n; o += gridDim.x, buf ^= 1) {
        long long li = indices != nullptr ? indices[o] : replay_draw(seed, step, stream_id, (unsigned long long)o, (unsigned long long)live);
        li = li < 0 ? 0 : li >= live ? live - 1 : li;      // never outside the window, whatever the caller passed
        const size_t slot = (size_t)((oldest + li) % ring.capacity);
        // everything the row needs is requested at once, behind the index alone: the history words and the policy entries
        // are loaded whether or not the meta word / the entry count (still in flight) will ask for them -- all 48 history
        // words and all 256 entries of a slot exist, the tail of the entries is zero -- and masked afterwards
        const uint32_t meta = ring.meta[slot];
        const int c = ring.cnt[slot];
        int pi = ring.idx[slot * HIVE_LIST_CAP + tid];
        const float pv = ring.val[slot * HIVE_LIST_CAP + tid];
        unsigned long long w = 0ull;
        uint32_t hw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        unsigned bit = 0u;
        if (tid < kCells) {
            unsigned wi;
            cell_word_bit((unsigned)tid, wi, bit);
            w = ring.feat[slot * kCells + tid];
            const uint32_t *h = ring.hist + slot * kHistWords + wi;
            HIVE_UNROLL for (int age = 0; age < 4; ++age) {
                hw[2 * age] = h[age * 12];
                hw[2 * age + 1] = h[age * 12 + 6];
            }
        }
        if (tid >= c) pi = -1;
        const unsigned hl = meta & 0xFFu, turn = (meta >> 8) & 0xFFu, mover = (meta >> 16) & 0xFFu;
        // the plane writer reads the history of perspective (turn odd ? 0 : 1); a packed row carries its MOVER's history, so
        // the planes 36..43 are there only where the two agree (records.dataset_tensors_gpu_packed fills the mover's half)
        const unsigned persp = (turn & 1u) ? 0u : 1u;
        const unsigned hlen = mover == persp ? (hl & 15u) : 0u;
        const uint32_t tv = PlaneVal<V>::of(turn);
        if (tid < kCells) {
            // history planes 36..43 = (own, enemy) occupancy 1..4 encodes ago
            HIVE_UNROLL for (unsigned age = 0; age < 4u; ++age)
                if (age < hlen) {
                    w |= (unsigned long long)((hw[2 * age] >> bit) & 1u) << (36u + 2u * age);
                    w |= (unsigned long long)((hw[2 * age + 1] >> bit) & 1u) << (37u + 2u * age);
                }
            full[buf][tid] = w;
        }
        {
            float4 *z = reinterpret_cast<float4 *>(pol[buf]);
            z[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tid < kPolPieces - 256) z[tid + 256] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if ((unsigned)pi < (unsigned)HIVE_ACTIONS) pol[buf][pi] = pv;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        plane_store_board<DT, LAYOUT, NT>(full[buf], one, tv, planes, o, tid);
        {
            // pieces tid, tid + 256 (< 396) of the row: consecutive lanes, consecutive 16 bytes
            const u32x4 *src = reinterpret_cast<const u32x4 *>(pol[buf]);
            u32x4 *dst = reinterpret_cast<u32x4 *>(policies + o * (long long)HIVE_ACTIONS);
            plane_store<NT>(src[tid], dst + tid);
            if (tid < kPolPieces - 256) plane_store<NT>(src[tid + 256], dst + tid + 256);
        }
        if (tid == 0) {
            values[o] = ring.value[slot];
            if (indices_out != nullptr) indices_out[o] = li;
        }
    }
}

Ring ring_of(const HiveReplay *r) { return Ring{r->feat, r->hist, r->meta, r->value, r->cnt, r->idx, r->val, r->capacity}; }

void advance(HiveReplay *r, long long rows)
{
    r->head = (r->head + rows) % r->capacity;
    r->live = std::min(r->live + rows, r->capacity);
    r->appended += rows;
}
}  // namespace

extern "C" int hive_replay_destroy(HiveReplay *r)
{
    if (!r) return HIVE_OK;
    (void)hipFree(r->feat);
    (void)hipFree(r->hist);
    (void)hipFree(r->meta);
    (void)hipFree(r->value);
    (void)hipFree(r->cnt);
    (void)hipFree(r->idx);
    (void)hipFree(r->val);
    (void)hipFree(r->discount);
    delete r;
    return HIVE_OK;
}

extern "C" int hive_replay_create(int device, int64_t capacity, const float *discount, HiveReplay **out)
{
    if (!out || capacity < 1 || capacity > (int64_t)0x7FFFFFFF)
        return hive::set_error(HIVE_E_ARG, "hive_replay_create: capacity 1 .. 2^31 - 1 rows");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
        return hive::set_error(HIVE_E_DEVICE, "hive_replay_create: no such HIP device");
    REPLAY_TRY(hipSetDevice(device));
    HiveReplay *r = new HiveReplay();
    r->device = device;
    r->capacity = capacity;
    const size_t cap = (size_t)capacity;
    float table[256];
    for (int k = 0; k < 256; ++k) table[k] = discount ? discount[k] : (float)std::pow(0.99, (double)k);
    hipError_t e = hipMalloc(&r->feat, sizeof(unsigned long long) * kCells * cap);
    if (e == hipSuccess) e = hipMalloc(&r->hist, sizeof(uint32_t) * kHistWords * cap);
    if (e == hipSuccess) e = hipMalloc(&r->meta, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc(&r->value, sizeof(float) * cap);
    if (e == hipSuccess) e = hipMalloc(&r->cnt, sizeof(int32_t) * cap);
    if (e == hipSuccess) e = hipMalloc(&r->idx, sizeof(int16_t) * HIVE_LIST_CAP * cap);
    if (e == hipSuccess) e = hipMalloc(&r->val, sizeof(float) * HIVE_LIST_CAP * cap);
    if (e == hipSuccess) e = hipMalloc(&r->discount, sizeof(table));
    if (e == hipSuccess) e = hipMemcpy(r->discount, table, sizeof(table), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hive_replay_destroy(r);
        return hive::set_error(HIVE_E_DEVICE, std::string("hive_replay_create: ") + hipGetErrorString(e));
    }
    *out = r;
    return HIVE_OK;
}

extern "C" int hive_replay_clear(HiveReplay *r, void *stream)
{
    (void)stream;                                          // the bookkeeping is on the host: nothing to launch
    if (!r) return hive::set_error(HIVE_E_ARG, "hive_replay_clear: null handle");
    r->head = 0;
    r->live = 0;
    return HIVE_OK;
}

extern "C" int hive_replay_stats(HiveReplay *r, int64_t *live, int64_t *appended, int64_t *capacity)
{
    if (!r) return hive::set_error(HIVE_E_ARG, "hive_replay_stats: null handle");
    if (live) *live = r->live;
    if (appended) *appended = r->appended;
    if (capacity) *capacity = r->capacity;
    return HIVE_OK;
}

extern "C" int hive_replay_append(HiveReplay *r, const uint64_t *feat, const uint32_t *hist, const uint8_t *meta,
                                  const int16_t *pol_idx, const float *pol_val, const int64_t *pol_ptr, const int64_t *game_ptr,
                                  const int8_t *game_val, const int64_t *pol_ptr_host, int64_t rows, int64_t games, void *stream)
{
    if (!r) return hive::set_error(HIVE_E_ARG, "hive_replay_append: null handle");
    if (rows < 0 || games < 0) return hive::set_error(HIVE_E_ARG, "hive_replay_append: negative count");
    if (rows == 0) return HIVE_OK;
    if (!feat || !hist || !meta || !pol_ptr || !game_ptr || !game_val || !pol_ptr_host || games == 0)
        return hive::set_error(HIVE_E_ARG, "hive_replay_append: null pointer (or no game) with rows > 0");
    long long entries = 0;
    for (int64_t i = 0; i < rows; ++i) {
        const long long c = (long long)(pol_ptr_host[i + 1] - pol_ptr_host[i]);
        if (c < 0 || c > HIVE_LIST_CAP)
            return hive::set_error(HIVE_E_ARG, "hive_replay_append: row " + std::to_string(i) + " has " + std::to_string(c) +
                                                   " policy entries (0 .. " + std::to_string(HIVE_LIST_CAP) + ")");
        entries += c;
    }
    if (entries > 0 && (!pol_idx || !pol_val)) return hive::set_error(HIVE_E_ARG, "hive_replay_append: null policy arrays");
    const long long skip = rows > r->capacity ? rows - r->capacity : 0;
    const unsigned blocks = (unsigned)std::min<long long>(rows - skip, kReplayMaxBlocks);
    hipLaunchKernelGGL((replay_write_kernel<true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, ring_of(r), r->head, skip,
                       (long long)rows, (long long)games, reinterpret_cast<const unsigned long long *>(feat), hist, meta, pol_idx,
                       pol_val, reinterpret_cast<const long long *>(pol_ptr), (const int32_t *)nullptr,
                       reinterpret_cast<const long long *>(game_ptr), game_val, (const float *)nullptr, r->discount,
                       (const long long *)nullptr, 0ll);
    REPLAY_TRY(hipGetLastError());
    advance(r, rows);
    return HIVE_OK;
}

extern "C" int hive_replay_append_ranked(HiveReplay *r, const uint64_t *feat, const uint32_t *hist, const uint8_t *meta,
                                         const int16_t *pol_idx, const float *pol_val, const int64_t *pol_ptr, const int64_t *game_ptr,
                                         const int8_t *game_val, const int64_t *pol_ptr_host, const int64_t *rank, int64_t rows,
                                         int64_t games, int64_t kept, void *stream)
{
    if (!r) return hive::set_error(HIVE_E_ARG, "hive_replay_append_ranked: null handle");
    if (rows < 0 || games < 0 || kept < 0 || kept > rows) return hive::set_error(HIVE_E_ARG, "hive_replay_append_ranked: bad count");
    if (rows == 0 || kept == 0) return HIVE_OK;
    if (!feat || !hist || !meta || !pol_ptr || !game_ptr || !game_val || !pol_ptr_host || !rank || games == 0)
        return hive::set_error(HIVE_E_ARG, "hive_replay_append_ranked: null pointer (or no game) with rows > 0");
    long long entries = 0;
    for (int64_t i = 0; i < rows; ++i) {
        const long long c = (long long)(pol_ptr_host[i + 1] - pol_ptr_host[i]);
        if (c < 0 || c > HIVE_LIST_CAP)
            return hive::set_error(HIVE_E_ARG, "hive_replay_append_ranked: row " + std::to_string(i) + " has " + std::to_string(c) +
                                                   " policy entries (0 .. " + std::to_string(HIVE_LIST_CAP) + ")");
        entries += c;
    }
    if (entries > 0 && (!pol_idx || !pol_val)) return hive::set_error(HIVE_E_ARG, "hive_replay_append_ranked: null policy arrays");
    const unsigned blocks = (unsigned)std::min<long long>(rows, kReplayMaxBlocks);
    hipLaunchKernelGGL((replay_write_kernel<true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, ring_of(r), r->head, 0ll,
                       (long long)rows, (long long)games, reinterpret_cast<const unsigned long long *>(feat), hist, meta, pol_idx,
                       pol_val, reinterpret_cast<const long long *>(pol_ptr), (const int32_t *)nullptr,
                       reinterpret_cast<const long long *>(game_ptr), game_val, (const float *)nullptr, r->discount,
                       reinterpret_cast<const long long *>(rank), (long long)(kept > r->capacity ? kept - r->capacity : 0));
    REPLAY_TRY(hipGetLastError());
    advance(r, kept);
    return HIVE_OK;
}

extern "C" int hive_replay_import(HiveReplay *r, const uint64_t *feat, const uint32_t *hist, const uint8_t *meta,
                                  const int32_t *pol_cnt, const int16_t *pol_idx, const float *pol_val, const float *values,
                                  int64_t rows, void *stream)
{
    if (!r) return hive::set_error(HIVE_E_ARG, "hive_replay_import: null handle");
    if (rows < 0) return hive::set_error(HIVE_E_ARG, "hive_replay_import: negative count");
    if (rows == 0) return HIVE_OK;
    if (!feat || !hist || !meta || !pol_cnt || !pol_idx || !pol_val || !values)
        return hive::set_error(HIVE_E_ARG, "hive_replay_import: null pointer with rows > 0");
    const long long skip = rows > r->capacity ? rows - r->capacity : 0;
    const unsigned blocks = (unsigned)std::min<long long>(rows - skip, kReplayMaxBlocks);
    hipLaunchKernelGGL((replay_write_kernel<false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, ring_of(r), r->head, skip,
                       (long long)rows, 0ll, reinterpret_cast<const unsigned long long *>(feat), hist, meta, pol_idx, pol_val,
                       (const long long *)nullptr, pol_cnt, (const long long *)nullptr, (const int8_t *)nullptr, values,
                       r->discount, (const long long *)nullptr, 0ll);
    REPLAY_TRY(hipGetLastError());
    advance(r, rows);
    return HIVE_OK;
}

extern "C" int hive_replay_export(HiveReplay *r, uint64_t *feat, uint32_t *hist, uint8_t *meta, int32_t *pol_cnt, int16_t *pol_idx,
                                  float *pol_val, float *values, void *stream)
{
    if (!r) return hive::set_error(HIVE_E_ARG, "hive_replay_export: null handle");
    if (r->live == 0) return HIVE_OK;
    const long long oldest = (r->head - r->live + r->capacity) % r->capacity;
    const unsigned blocks = (unsigned)std::min<long long>(r->live, kReplayMaxBlocks);
    hipLaunchKernelGGL(replay_export_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ring_of(r), oldest, r->live,
                       reinterpret_cast<unsigned long long *>(feat), hist, meta, pol_cnt, pol_idx, pol_val, values);
    REPLAY_TRY(hipGetLastError());
    REPLAY_TRY(hipStreamSynchronize((hipStream_t)stream));
    return HIVE_OK;
}

extern "C" int hive_replay_sample(HiveReplay *r, const int64_t *indices, uint64_t seed, uint64_t step, uint64_t stream_id, int n,
                                  HiveDType dtype, HiveLayout layout, void *planes, float *policies, float *values,
                                  int64_t *indices_out, void *stream)
{
    if (!r || n <= 0 || !planes || !policies || !values) return hive::set_error(HIVE_E_ARG, "hive_replay_sample: n <= 0 or a NULL buffer");
    const int dt = (int)dtype, ly = (int)layout;
    if (dt < 0 || dt > 2 || ly < 0 || ly > 1) return hive::set_error(HIVE_E_ARG, "hive_replay_sample: unknown dtype/layout");
    if (((uintptr_t)planes | (uintptr_t)policies) & 15u)
        return hive::set_error(HIVE_E_ARG, "hive_replay_sample: planes and policies must be 16-byte aligned");
    if (r->live == 0) return hive::set_error(HIVE_E_STATE, "hive_replay_sample: the window is empty");
    const long long oldest = (r->head - r->live + r->capacity) % r->capacity;
    const dim3 grid((unsigned)std::min<long long>(n, kReplayMaxBlocks));
    const long long *idx = reinterpret_cast<const long long *>(indices);
    long long *idx_out = reinterpret_cast<long long *>(indices_out);
#define HIVE_SAMPLE_CASE(DT, LY)                                                                                          \
    if (dt == DT && ly == LY) {                                                                                           \
        if (n >= kExpandStreamBoards)                                                                                     \
            hipLaunchKernelGGL((replay_sample_kernel<DT, LY, true>), grid, dim3(256), 0, (hipStream_t)stream, ring_of(r), oldest, \
                               r->live, idx, (unsigned long long)seed, (unsigned long long)step, (unsigned long long)stream_id, n, \
                               planes, policies, values, idx_out);                                                        \
        else                                                                                                              \
            hipLaunchKernelGGL((replay_sample_kernel<DT, LY, false>), grid, dim3(256), 0, (hipStream_t)stream, ring_of(r), oldest, \
                               r->live, idx, (unsigned long long)seed, (unsigned long long)step, (unsigned long long)stream_id, n, \
                               planes, policies, values, idx_out);                                                        \
    }
    HIVE_SAMPLE_CASE(0, 0) HIVE_SAMPLE_CASE(0, 1) HIVE_SAMPLE_CASE(1, 0) HIVE_SAMPLE_CASE(1, 1) HIVE_SAMPLE_CASE(2, 0) HIVE_SAMPLE_CASE(2, 1)
#undef HIVE_SAMPLE_CASE
    REPLAY_TRY(hipGetLastError());
    return HIVE_OK;
}
