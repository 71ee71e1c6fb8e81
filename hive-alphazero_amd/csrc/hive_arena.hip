// hive_arena.hip -- net-vs-net matches (woker/evaluation.py): the two sides of a game are searched with different
// networks, both networks share one leaf batch.
//
// Every row of a leaf batch belongs to the network of the side to move AT THE ROOT of its game (a search is one player's
// thinking: HivePlayer.action evaluates every position of its tree with its own model, whoever is to move in it).
//   hive_arena_split_launch    the need flags of hive_search_leaf_need, split by owner: each network's tower runs only
//                              over its own rows
//   hive_arena_budget_launch   the simulations each game's search gets when the two sides search unequally
//   hive_arena_join_launch     B's rows of (p, v) copied over A's: one (p, v) pair for hive_search_backup
//   hive_arena_opening_launch  the uniformly random opening moves (evaluation.py:169,187), keyed on (seed, pair, turn):
//                              both games of a pair play the same opening
//   hive_arena_score_launch    finished games -> result per game + the match tally
// Byte-wide flags are written one lane per row; counters are added to with vector atomics, one per wave.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/hive_search.h"
#include "hive_rng.hpp"

namespace hive {
int set_error(int code, const std::string &msg);
}

namespace {
constexpr int kPolicy = HIVE_ACTIONS;                 // floats per policy row
constexpr int kRowVec = kPolicy * 4 / 16;             // 16-byte words per policy row
static_assert(kPolicy * 4 % 16 == 0, "policy rows are copied in 16-byte words");

#define ARENA_TRY(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return hive::set_error(HIVE_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// network A owns the search of game g iff A's colour is the colour to move at the root (odd turn = white)
__device__ __forceinline__ bool owner_is_a(const HiveBoard *__restrict__ roots, const int8_t *__restrict__ a_white, int g)
{
    return (a_white[g] != 0) == ((roots[g].turn & 1) != 0);
}

// one lane per row
__global__ void __launch_bounds__(256)
arena_split_kernel(const HiveBoard *__restrict__ roots, const int8_t *__restrict__ a_white, const int8_t *__restrict__ need,
                   int games, int n, int8_t *__restrict__ need_a, int8_t *__restrict__ need_b,
                   unsigned long long *__restrict__ rows_a, unsigned long long *__restrict__ rows_b)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    bool fa = false, fb = false;
    if (r < n) {
        const bool wanted = need ? need[r] != 0 : true;
        const bool a = owner_is_a(roots, a_white, r % games);
        fa = wanted && a;
        fb = wanted && !a;
        need_a[r] = fa ? 1 : 0;
        need_b[r] = fb ? 1 : 0;
    }
    const unsigned long long ba = __ballot(fa), bb = __ballot(fb);
    if ((threadIdx.x & 63) == 0) {
        if (rows_a && ba) atomicAdd(rows_a, (unsigned long long)__popcll(ba));
        if (rows_b && bb) atomicAdd(rows_b, (unsigned long long)__popcll(bb));
    }
}

// one lane per game
__global__ void __launch_bounds__(256)
arena_budget_kernel(const HiveBoard *__restrict__ roots, const int8_t *__restrict__ a_white, int games, int sims_a, int sims_b,
                    int32_t *__restrict__ budget)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= games) return;
    budget[g] = owner_is_a(roots, a_white, g) ? sims_a : sims_b;
}

// one wave per row
__global__ void __launch_bounds__(256)
arena_join_kernel(const HiveBoard *__restrict__ roots, const int8_t *__restrict__ a_white, int games, int n,
                  float *__restrict__ p_a, float *__restrict__ v_a, const float *__restrict__ p_b, const float *__restrict__ v_b)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    if (owner_is_a(roots, a_white, r % games)) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(p_b + (size_t)r * kPolicy);
    uint4 *dst = reinterpret_cast<uint4 *>(p_a + (size_t)r * kPolicy);
    for (int i = lane; i < kRowVec; i += 64) dst[i] = src[i];
    if (lane == 0) v_a[r] = v_b[r];
}

// one lane per game
__global__ void __launch_bounds__(256)
arena_opening_kernel(const HiveBoard *__restrict__ boards, const int32_t *__restrict__ count, const int16_t *__restrict__ list,
                     const long long *__restrict__ pair_id, const int8_t *__restrict__ active, int n, unsigned long long seed,
                     int opening_turns, int32_t *__restrict__ action)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    if (active && !active[g]) return;
    const unsigned turn = boards[g].turn;
    if ((int)turn > opening_turns) return;
    int c = count[g];
    if (c > HIVE_LIST_CAP) c = HIVE_LIST_CAP;
    if (c <= 0) { action[g] = -1; return; }
    const unsigned long long r = hive::splitmix(hive::Rng(seed, (unsigned long long)pair_id[g], (unsigned long long)turn, 0ull).s);
    const unsigned idx = (unsigned)(((r >> 32) * (unsigned long long)c) >> 32);      // < c
    action[g] = (int32_t)list[(size_t)g * HIVE_LIST_CAP + idx];
}

__device__ __forceinline__ int wave_sum_int(int x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// one lane per game; tally: [0] A wins as white [1] A wins as black [2] B wins as white [3] B wins as black [4] draws
// [5] length cap [6] finished games [7] summed final turn
__global__ void __launch_bounds__(256)
arena_score_kernel(const HiveBoard *__restrict__ boards, const int8_t *__restrict__ over, const int8_t *__restrict__ winner,
                   const int8_t *__restrict__ active, const int8_t *__restrict__ a_white, int n, int max_game_length,
                   int8_t *__restrict__ result, int32_t *__restrict__ tally)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    int kind = -1, turn = 0;
    if (g < n) {
        int res = 0;
        turn = boards[g].turn;
        const bool on = active ? active[g] != 0 : true;
        if (on && over[g]) {
            const int w = winner[g];
            const bool aw = a_white[g] != 0;
            if (w == 1) { kind = aw ? 0 : 2; res = aw ? 1 : 2; }
            else if (w == 2) { kind = aw ? 3 : 1; res = aw ? 2 : 1; }
            else { kind = 4; res = 3; }
        } else if (on && turn >= max_game_length) {
            kind = 5;
            res = 4;
        }
        result[g] = (int8_t)res;
    }
    if (kind < 0) turn = 0;
    const int turns = wave_sum_int(turn);
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < 6; ++k) {
        const unsigned long long b = __ballot(kind == k);
        if (lane == 0 && b) atomicAdd(&tally[k], (int)__popcll(b));
    }
    const unsigned long long done = __ballot(kind >= 0);
    if (lane == 0 && done) {
        atomicAdd(&tally[6], (int)__popcll(done));
        atomicAdd(&tally[7], turns);
    }
}
}  // namespace

extern "C" int hive_arena_split_launch(const HiveBoard *root_boards, const int8_t *a_white, const int8_t *need, int games, int slots,
                                       int8_t *need_a, int8_t *need_b, uint64_t *rows_a, uint64_t *rows_b, void *stream)
{
    if (!root_boards || !a_white || !need_a || !need_b || games <= 0 || slots <= 0 || slots > HIVE_MAX_SLOTS ||
        (long long)games * slots > 0x7fffffffll)
        return hive::set_error(HIVE_E_ARG, "hive_arena_split_launch: bad argument (games >= 1, 1 <= slots <= HIVE_MAX_SLOTS)");
    const int n = games * slots;
    hipLaunchKernelGGL(arena_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, root_boards, a_white,
                       need, games, n, need_a, need_b, reinterpret_cast<unsigned long long *>(rows_a),
                       reinterpret_cast<unsigned long long *>(rows_b));
    ARENA_TRY(hipGetLastError());
    return HIVE_OK;
}

extern "C" int hive_arena_budget_launch(const HiveBoard *root_boards, const int8_t *a_white, int games, int sims_a, int sims_b,
                                        int32_t *budget, void *stream)
{
    if (!root_boards || !a_white || !budget || games <= 0 || sims_a < 0 || sims_b < 0)
        return hive::set_error(HIVE_E_ARG, "hive_arena_budget_launch: bad argument");
    hipLaunchKernelGGL(arena_budget_kernel, dim3((unsigned)((games + 255) / 256)), dim3(256), 0, (hipStream_t)stream, root_boards,
                       a_white, games, sims_a, sims_b, budget);
    ARENA_TRY(hipGetLastError());
    return HIVE_OK;
}

extern "C" int hive_arena_join_launch(const HiveBoard *root_boards, const int8_t *a_white, int games, int slots, float *p_a, float *v_a,
                                      const float *p_b, const float *v_b, void *stream)
{
    if (!root_boards || !a_white || !p_a || !v_a || !p_b || !v_b || games <= 0 || slots <= 0 || slots > HIVE_MAX_SLOTS ||
        (long long)games * slots > 0x7fffffffll)
        return hive::set_error(HIVE_E_ARG, "hive_arena_join_launch: bad argument (games >= 1, 1 <= slots <= HIVE_MAX_SLOTS)");
    if (((uintptr_t)p_a | (uintptr_t)p_b) & 15u)
        return hive::set_error(HIVE_E_ARG, "hive_arena_join_launch: the policy arrays must be 16-byte aligned");
    const int n = games * slots;
    hipLaunchKernelGGL(arena_join_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, root_boards, a_white, games,
                       n, p_a, v_a, p_b, v_b);
    ARENA_TRY(hipGetLastError());
    return HIVE_OK;
}

extern "C" int hive_arena_opening_launch(const HiveBoard *boards, const int32_t *count, const int16_t *list, const int64_t *pair_id,
                                         const int8_t *active, int n, uint64_t seed, int opening_turns, int32_t *action, void *stream)
{
    if (!boards || !count || !list || !pair_id || !action || n <= 0)
        return hive::set_error(HIVE_E_ARG, "hive_arena_opening_launch: bad argument");
    hipLaunchKernelGGL(arena_opening_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boards, count, list,
                       reinterpret_cast<const long long *>(pair_id), active, n, (unsigned long long)seed, opening_turns, action);
    ARENA_TRY(hipGetLastError());
    return HIVE_OK;
}

extern "C" int hive_arena_score_launch(const HiveBoard *boards, const int8_t *over, const int8_t *winner, const int8_t *active,
                                       const int8_t *a_white, int n, int max_game_length, int8_t *result, int32_t *tally, void *stream)
{
    if (!boards || !over || !winner || !a_white || !result || !tally || n <= 0)
        return hive::set_error(HIVE_E_ARG, "hive_arena_score_launch: bad argument");
    hipLaunchKernelGGL(arena_score_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boards, over, winner,
                       active, a_white, n, max_game_length, result, tally);
    ARENA_TRY(hipGetLastError());
    return HIVE_OK;
}
