// hive_search.hip -- GPU-resident PUCT tree search over thousands of concurrent Hive games.
//
// Flat SoA node pool in HBM, one tree per game, one wavefront per game per kernel: lanes stride
// over a node's edges, so the per-edge arrays (prior, visits, value sum, child) are read with
// coalesced 256-byte wave loads; argmax / sums are wave reductions.  See include/hive_search.h
// for the reference functions each entry point replaces.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/hive_search.h"
#include "hive_rng.hpp"
#include "hive_step.hpp"

namespace hive {

constexpr int EC = HIVE_EDGE_CAP;
enum LeafKind : int8_t { LEAF_NONE = 0, LEAF_ROOT = 1, LEAF_EXPAND = 2, LEAF_TERMINAL = 3, LEAF_COLLISION = 4, LEAF_CAPDRAW = 5,
                  LEAF_PROVEN = 8 /* descent ended at a proven node (hive_search_set_solver); histogram bucket [3] */ };
constexpr float kDrawSentinel = 5.0f;      // solo_play.py:180,183

struct SearchDev {
    int G, MN, L;
    HiveSearchParams prm;
    unsigned long long seed;
    HiveBoard *node_board;
    HiveHistory *node_hist;
    int32_t *node_nedge, *node_sum_n;
    int8_t *node_term;
    float *node_tv;
    float *node_v;                                 // [G][MN] value the node was created with: the network's (side to move), or tv
    int16_t *e_act;
    float *e_p, *e_w;
    int32_t *e_n, *e_child;
    int32_t *n_nodes;
    int8_t *active, *root_pending;
    HiveBoard *root_board;
    HiveHistory *root_hist;
    int32_t *path_node, *path_edge, *path_len;     // [L][G][MN], [L][G]
    int8_t *leaf_kind;                             // [L][G]
    int32_t *leaf_node;                            // [L][G]: terminal node reached / parent node of the expansion
    int32_t *leaf_edge;                            // [L][G]: parent edge of the expansion
    int32_t *tt;                                   // [G][TT] open-addressing table position -> node (-1 empty)
    int32_t *tt_hits;                              // [G] descents that continued through a transposition (statistics)
    int TT, merge;                                 // table size (power of two), merging on/off
    long long *game_id;                            // [G] global game index: the only per-game key of the noise streams
    int32_t *kind_hist;                            // [G][8] leaves by LeafKind since create (statistics)
    int32_t *carry_kept, *carry_visits, *carry_refused;   // [G] hive_search_carry_stats
    int sims_room;                                 // nodes a carried tree must leave free (hive_search_set_carry_room)
    const int32_t *budget;                         // [G] simulations of this search per game, or nullptr (hive_search_set_budgets)
    const int8_t *quiet;                           // [G] != 0: no root noise for that game, or nullptr
    int32_t *clock;                                // [G] simulations of its own search each game has run, or nullptr: one
                                                   // host counter for the whole batch (hive_search_set_rolling)
    float *root_v;                                 // [G] the network's value of the root position (search_backup_kernel, LEAF_ROOT)
    int gum_on;                                    // hive_search_set_gumbel: the Gumbel root is on ...
    HiveGumbelParams gum;
    const int8_t *gum_where;                       // ... for the games with gum_where[g] != 0 (nullptr: for every game)
    int32_t *gum_fallback;                         // [G] root selections that found no edge at the scheduled visit count
    int gum_int_on;                                // hive_search_set_gumbel_interior: Gumbel games descend by the interior rule ...
    const int8_t *gum_int_where;                   // ... where gum_int_where[g] != 0 (nullptr: every Gumbel game)
    int solver_on;                                 // hive_search_set_solver: proven wins and losses are on ...
    const int8_t *solver_where;                    // ... for the games with solver_where[g] != 0 (nullptr: for every game)
    int8_t *node_status, *e_status;                // [G][MN], [G][MN][EC]; nullptr until the option is first switched on
    int32_t *solver_stats;                         // [G][4] hive_search_solver_stats
};

// the node arrays of one pool: hive_search_advance_roots moves the kept subtrees from the handle's pool into a second one
struct NodePool {
    HiveBoard *node_board;
    HiveHistory *node_hist;
    int32_t *node_nedge, *node_sum_n;
    int8_t *node_term;
    float *node_tv;
    float *node_v;
    int16_t *e_act;
    float *e_p, *e_w;
    int32_t *e_n, *e_child;
    int8_t *node_status, *e_status;                // nullptr until hive_search_set_solver allocates them
};

// ------------------------------------------------------------------ small device helpers
// splitmix / Rng: the counter-based generator (hive_rng.hpp, shared with hive_arena.hip)

// noise key of one draw: (search seed, global game id, turn of the root position, simulation of this search, in-flight
// slot, edge) -- nothing that depends on where in a batch, on which GPU or after how many other searches the game runs
__device__ __forceinline__ Rng noise_rng(unsigned long long seed, long long game, unsigned turn, unsigned long long sim,
                                         int slot, int e)
{
    return Rng(seed, (unsigned long long)game, ((unsigned long long)turn << 40) | (sim * 8ull + (unsigned long long)slot),
               (unsigned long long)e);
}

__device__ __forceinline__ float wave_sum(float x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float wave_max(float x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ int wave_sum_i(int x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
// (score, index) argmax; ties go to the lower index (first max wins, solo_play.py:332-334)
__device__ __forceinline__ void wave_argmax(float &score, int &idx)
{
    for (int o = 32; o > 0; o >>= 1) {
        float s2 = __shfl_xor(score, o);
        int i2 = __shfl_xor(idx, o);
        if (s2 > score || (s2 == score && i2 < idx)) { score = s2; idx = i2; }
    }
}
__device__ __forceinline__ void wave_copy(void *dst, const void *src, int bytes, int lane)
{
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (int i = lane; i < bytes / 4; i += 64) d[i] = s[i];
}

// eta ~ Dirichlet(alpha) over the ne edges of one node, edge e = lane + 64 k in noise[k] (np.random.dirichlet,
// solo_play.py:322-323): independent Gamma(alpha, 1) draws divided by their sum
__device__ __forceinline__ void wave_dirichlet(float noise[4], int ne, float alpha, unsigned long long seed, long long game,
                                               unsigned turn, unsigned long long sim, int slot, int lane)
{
    float tot = 0.f;
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        noise[k] = 0.f;
        if (e < ne) {
            Rng r = noise_rng(seed, game, turn, sim, slot, e);
            noise[k] = r.gamma(alpha);
            tot += noise[k];
        }
    }
    tot = wave_sum(tot);
    const float inv = tot > 0.f ? 1.0f / tot : 0.f;
    for (int k = 0; k < 4; ++k) noise[k] *= inv;
}

// child_Q() + child_U() of alpha_zero/MCTS_chess.py:52-57 for one edge, in the reference's fp32 operation order
// (numpy float32 arrays; math.sqrt(number_visits) enters as a float32 scalar): W/(1+N) + sqrtN * (|P|/(1+N)).
// No fused multiply-add: the sum must round like numpy's separate multiply and add.
__device__ __forceinline__ float uct_score(float w, float n, float p, float sqrt_visits)
{
#pragma clang fp contract(off)
    const float d = 1.0f + n;
    const float q = w / d;
    const float u = sqrt_visits * (fabsf(p) / d);
    return q + u;
}

// ------------------------------------------------------------------ Gumbel root (include/hive_search.h, hive_search_set_gumbel)
constexpr unsigned long long kGumbelStream = 0x6A09E667F3BCC909ull;

__device__ __forceinline__ bool gumbel_game(const SearchDev &S, int g)
{
    return S.gum_on && S.prm.mode != HIVE_SEARCH_UCT && (S.gum_where == nullptr || S.gum_where[g] != 0);
}

// ------------------------------------------------------------------ proven wins and losses (include/hive_search.h, hive_search_set_solver)
__device__ __forceinline__ bool solver_game(const SearchDev &S, int g)
{
    return S.solver_on && S.prm.mode != HIVE_SEARCH_UCT && (S.solver_where == nullptr || S.solver_where[g] != 0);
}
// a status holds on a path whose current turn is `turn` iff the finished position lies within the length cap
__device__ __forceinline__ bool solver_holds(int x, int turn, int cap)
{
    return x != 0 && turn + (x < 0 ? -x : x) - 1 <= cap;
}
// lanes of one wave see each other's LDS / global writes made before this point
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// The statuses of a node's edges, four per lane (edge e = lane + 64 k in es[k], 0 past the last edge), `own` standing in
// for edge `at` (the one this backup just wrote): the node's status -- the fastest win if any edge wins, the longest
// resistance if every edge loses, else unknown.
__device__ __forceinline__ int wave_solver_node_status(const int8_t *es_row, int ne, int at, int own, int lane)
{
    int minpos = 128, maxabs = 0;
    bool open = false;                                       // an edge of mine that is not a proven loss
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        if (e < ne) {
            const int x = e == at ? own : (int)es_row[e];
            if (x > 0 && x < minpos) minpos = x;
            if (x >= 0) open = true;
            if (-x > maxabs) maxabs = -x;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(minpos, o), b = __shfl_xor(maxabs, o);
        minpos = a < minpos ? a : minpos;
        maxabs = b > maxabs ? b : maxabs;
    }
    if (minpos < 128) return minpos;
    return __ballot(open) == 0ull ? -maxabs : 0;
}

// entry i of the sequential-halving sequence of considered visits for m >= 1 considered actions and n simulations: the
// phases are walked arithmetically.  In a phase the first k slots all hold the same count `base` (k only shrinks, and every
// emission increments all of the first k), so a phase is `extra` runs of k equal entries base, base + 1, ...
__device__ __forceinline__ int gumbel_considered_visit(int m, int n, int i)
{
    if (m <= 1) return i;
    int L = 0;
    while ((1 << L) < m) ++L;
    int k = m, base = 0, pos = 0;
    while (true) {                                              // every phase emits at least 2 entries: at most i / 2 rounds
        int extra = n / (L * k);
        if (extra < 1) extra = 1;
        const int len = extra * k;
        if (i < pos + len) return base + (i - pos) / k;
        pos += len;
        base += extra;
        k = k / 2 > 2 ? k / 2 : 2;
    }
}

// sigma(q~) and the score of one edge, fp32 without contraction like uct_score
__device__ __forceinline__ float gumbel_sigma(float c_visit, float c_scale, float max_n, float qn)
{
#pragma clang fp contract(off)
    return (c_visit + max_n) * c_scale * qn;
}
__device__ __forceinline__ float gumbel_score(float g, float logit, float sigma)
{
#pragma clang fp contract(off)
    const float a = g + logit;
    return a + sigma;
}
// below the root: how far the edge's visit share lags the improved policy (hive_search_set_gumbel_interior)
__device__ __forceinline__ float gumbel_interior_score(float improved, int n, int sum_n)
{
#pragma clang fp contract(off)
    return improved - (float)n / (1.0f + (float)sum_n);
}

// The per-edge quantities of a Gumbel node, edge e = lane + 64 k in slot k: g, logit, completed q, sigma and the visits.
// v_node = the network's value of the node's own position (root_v at the root, node_v below it); draw = the g of a root
// that is not quiet, else g = 0.  nv[k] = -1 marks a slot past the last edge.  max_n / sum_n are wave-uniform.
__device__ __forceinline__ void wave_gumbel_root(const SearchDev &S, int g, long long eb, int ne, unsigned root_turn, float v_node,
                                                 bool draw, int lane, float gum[4], float logit[4], float qhat[4], float sigma[4],
                                                 int nv[4], int &max_n, int &sum_n)
{
    int nsum = 0, nmax = 0;
    float pq = 0.f, pv = 0.f;
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        gum[k] = logit[k] = qhat[k] = sigma[k] = 0.f;
        nv[k] = -1;
        if (e < ne) {
            const float p = S.e_p[eb + e];
            const int n = S.e_n[eb + e];
            nv[k] = n;
            logit[k] = logf(fmaxf(p, 1e-30f));
            if (draw) {
                Rng r = noise_rng(S.seed ^ kGumbelStream, S.game_id[g], root_turn, 0ull, 0, e);
                gum[k] = -logf(-logf(r.uniform()));
            }
            if (n > 0) {
                qhat[k] = S.e_w[eb + e] / (float)n;
                pq += p * qhat[k];
                pv += p;
                nsum += n;
                nmax = n > nmax ? n : nmax;
            }
        }
    }
    nsum = wave_sum_i(nsum);
    for (int o = 32; o > 0; o >>= 1) { const int x = __shfl_xor(nmax, o); nmax = x > nmax ? x : nmax; }
    pq = wave_sum(pq);
    pv = wave_sum(pv);
    // (visited edges whose priors are all zero -- the pass edge -- leave the mixed value at the node's own)
    const float v_mix = (nsum == 0 || !(pv > 0.f)) ? v_node : (v_node + (float)nsum * (pq / pv)) / (1.0f + (float)nsum);
    float lo = 3.0e38f, hi = -3.0e38f;
    for (int k = 0; k < 4; ++k)
        if (nv[k] >= 0) {
            if (nv[k] == 0) qhat[k] = v_mix;
            lo = fminf(lo, qhat[k]);
            hi = fmaxf(hi, qhat[k]);
        }
    hi = wave_max(hi);
    lo = -wave_max(-lo);
    const float span = fmaxf(hi - lo, 1e-8f);
    for (int k = 0; k < 4; ++k)
        if (nv[k] >= 0) sigma[k] = gumbel_sigma(S.gum.c_visit, S.gum.c_scale, (float)nmax, (qhat[k] - lo) / span);
    max_n = nmax;
    sum_n = nsum;
}

// softmax(logit + sigma) over the edges of one root: improved[k] for edge lane + 64 k (0 past the last edge)
__device__ __forceinline__ void wave_gumbel_improved(const float logit[4], const float sigma[4], const int nv[4], float improved[4])
{
    float mx = -3.0e38f;
    for (int k = 0; k < 4; ++k)
        if (nv[k] >= 0) mx = fmaxf(mx, logit[k] + sigma[k]);
    mx = wave_max(mx);
    float tot = 0.f;
    for (int k = 0; k < 4; ++k) {
        improved[k] = nv[k] >= 0 ? expf(logit[k] + sigma[k] - mx) : 0.f;
        tot += improved[k];
    }
    tot = wave_sum(tot);
    const float inv = tot > 0.f ? 1.0f / tot : 0.f;
    for (int k = 0; k < 4; ++k) improved[k] *= inv;
}

// The reference keeps its tree in a dict keyed by GamePlay.state_key (solo_play.py:167-197, env_hive.py:70-94,151-168):
// cells in board order with the piece keys bottom->top plus the side digit -- turn number and history excluded.
// The same information is bytes 0..32 of the HiveBoard record (pos[22], 4-bit stack indices) and the turn parity.
__device__ __forceinline__ uint32_t key_word(const uint32_t *rec, int i)      // i = 0..8
{
    uint32_t w = rec[i];
    if (i == 8) w = (w & 0xFFu) | ((w >> 8) & 1u) << 8;       // lvl[10] and the parity of the turn byte
    return w;
}
__device__ __forceinline__ uint32_t key_hash(const uint32_t *rec, int lane)
{
    unsigned long long h = 0ull;
    if (lane < 9) h = splitmix(((unsigned long long)(lane + 1) << 32) | key_word(rec, lane));
    for (int o = 8; o > 0; o >>= 1) h ^= __shfl_xor(h, o);      // lanes 0..15 hold the xor of lanes 0..8 (others add 0)
    return (uint32_t)(__shfl(h, 0) >> 17);
}
__device__ __forceinline__ bool key_equal(const uint32_t *a, const uint32_t *b, int lane)
{
    bool ne = lane < 9 && key_word(a, lane) != key_word(b, lane);
    return __ballot(ne) == 0ull;
}
// node holding the position `rec` of game g, or -1
__device__ __forceinline__ int tt_find(const SearchDev &S, int g, const uint32_t *rec, int lane)
{
    const uint32_t mask = (uint32_t)S.TT - 1u;
    uint32_t slot = key_hash(rec, lane) & mask;
    for (int probe = 0; probe < S.TT; ++probe, slot = (slot + 1u) & mask) {
        const int id = S.tt[(long long)g * S.TT + slot];
        if (id < 0) return -1;
        if (key_equal(rec, reinterpret_cast<const uint32_t *>(&S.node_board[(long long)g * S.MN + id]), lane)) return id;
    }
    return -1;
}
__device__ __forceinline__ void tt_insert(const SearchDev &S, int g, const uint32_t *rec, int id, int lane)
{
    const uint32_t mask = (uint32_t)S.TT - 1u;
    uint32_t slot = key_hash(rec, lane) & mask;
    for (int probe = 0; probe < S.TT; ++probe, slot = (slot + 1u) & mask)
        if (S.tt[(long long)g * S.TT + slot] < 0) {
            if (lane == 0) S.tt[(long long)g * S.TT + slot] = id;
            return;
        }
}

// ------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(256)
search_reset_kernel(SearchDev S, const int8_t *__restrict__ which, const HiveBoard *__restrict__ boards,
                    const HiveHistory *__restrict__ hist, const int8_t *__restrict__ active)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S.G) return;
    if (which != nullptr && which[g] == 0) return;          // hive_search_restart: every other game keeps every byte
    wave_copy(&S.root_board[g], &boards[g], sizeof(HiveBoard), lane);
    wave_copy(&S.root_hist[g], &hist[g], sizeof(HiveHistory), lane);
    for (int i = lane; i < S.TT; i += 64) S.tt[(long long)g * S.TT + i] = -1;
    if (lane == 0) {
        S.n_nodes[g] = 0;
        S.root_pending[g] = 0;
        S.active[g] = active ? active[g] : 1;
        if (S.clock != nullptr) S.clock[g] = 0;
    }
}

// solo_play.py:167-215 (descent), :294-335 (PUCT with per-simulation root noise)
__global__ void __launch_bounds__(256)
search_select_kernel(SearchDev S, int slot, unsigned long long sim, HiveBoard *__restrict__ leaf_boards,
                     HiveHistory *__restrict__ leaf_hist)
{
    __shared__ uint32_t stage[4][112];
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S.G) return;
    const long long sg = (long long)slot * S.G + g;
    int32_t *pnode = S.path_node + sg * S.MN, *pedge = S.path_edge + sg * S.MN;
    // a game whose budget is spent sits the rest of the search out exactly like an inactive one: no leaf, no virtual loss
    bool spent;
    if (S.clock != nullptr) {
        // rolling: the game's own clock numbers its simulations -- 0 alone, then `slots` per round (TreeSearch's layout)
        const int c = S.clock[g];
        spent = !(c + slot < S.budget[g] && (c > 0 || slot == 0));
        sim = (unsigned long long)(c + slot);
    } else {
        spent = S.budget != nullptr && (long long)sim >= (long long)S.budget[g];
    }
    if (!S.active[g] || spent) { if (lane == 0) { S.leaf_kind[sg] = LEAF_NONE; S.path_len[sg] = 0; } return; }

    if (S.n_nodes[g] == 0) {
        // first simulation of a search only evaluates the root (solo_play.py:188-197)
        int kind = S.root_pending[g] ? LEAF_COLLISION : LEAF_ROOT;
        if (kind == LEAF_ROOT) {
            wave_copy(&leaf_boards[g], &S.root_board[g], sizeof(HiveBoard), lane);
            wave_copy(&leaf_hist[g], &S.root_hist[g], sizeof(HiveHistory), lane);
        }
        if (lane == 0) { S.leaf_kind[sg] = (int8_t)kind; S.path_len[sg] = 0; S.root_pending[g] = 1; }
        return;
    }

    const long long nbase = (long long)g * S.MN;
    // The env of this simulation (deepcopy(env) of solo_play.py:158) lives in LDS and takes every move of the descent
    // (env.move, solo_play.py:213): turn number and history planes are those of THIS path even when the nodes it runs
    // through were first reached another way.
    uint32_t *st = stage[threadIdx.x >> 6];
    wave_copy(st, &S.node_board[nbase], sizeof(HiveBoard), lane);
    wave_copy(st + 16, &S.node_hist[nbase], sizeof(HiveHistory), lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    int node = 0, depth = 0, kind = LEAF_NONE, leafnode = 0, leafedge = 0;
    const unsigned root_turn = reinterpret_cast<const uint8_t *>(st)[33];
    const bool quiet = S.quiet != nullptr && S.quiet[g] != 0;
    const bool gumbel = gumbel_game(S, g);
    const bool interior = gumbel && S.gum_int_on && (S.gum_int_where == nullptr || S.gum_int_where[g] != 0);
    const bool solver = solver_game(S, g);
    while (true) {
        if (S.node_term[nbase + node]) { kind = LEAF_TERMINAL; leafnode = node; break; }          // game over (solo_play.py:169-180)
        if ((int)reinterpret_cast<const uint8_t *>(st)[33] >= S.prm.max_game_length) { kind = LEAF_CAPDRAW; break; }   // :181-183
        unsigned banned = 0u;                                // bit k: edge lane + 64 k is a proven loss that holds here
        if (solver) {
            // a proven node ends the descent like a finished game; at a node passed through, the moves proven to lose are
            // left out unless every move is one
            const int turn = (int)reinterpret_cast<const uint8_t *>(st)[33];
            if (solver_holds(S.node_status[nbase + node], turn, S.prm.max_game_length)) { kind = LEAF_PROVEN; leafnode = node; break; }
            const int ne_s = S.node_nedge[nbase + node];
            const int8_t *es = S.e_status + (nbase + node) * EC;
            bool open = false;
            for (int k = 0; k < 4; ++k) {
                const int e = lane + 64 * k;
                if (e < ne_s) {
                    const int x = es[e];
                    if (x < 0 && solver_holds(x, turn, S.prm.max_game_length)) banned |= 1u << k;
                    else open = true;
                }
            }
            if (__ballot(open) == 0ull) banned = 0u;
        }
        const int ne = S.node_nedge[nbase + node];
        const long long eb = (nbase + node) * EC;
        const bool uct = S.prm.mode == HIVE_SEARCH_UCT;
        // PUCT: sqrt(sum_n + 1) (solo_play.py:316).  UCT: sqrt(number_visits) of this node (MCTS_chess.py:55-57) -- every
        // backup through a node passes one of its edges except the one that expanded it, so number_visits = sum_n + 1 too
        const float xx = sqrtf((float)S.node_sum_n[nbase + node] + 1.0f);
        // fresh Dirichlet noise on the root priors for every simulation (solo_play.py:322-323)
        float noise[4] = {0.f, 0.f, 0.f, 0.f};
        const bool noisy = depth == 0 && !uct && S.prm.noise_eps > 0.f && !quiet && !gumbel;
        if (noisy)
            wave_dirichlet(noise, ne, S.prm.dirichlet_alpha, S.seed, S.game_id[g], root_turn, sim, slot, lane);
        float best = -3.0e38f;
        int bidx = 0x7FFFFFFF;
        if (depth == 0 && gumbel) {
            // Gumbel root: simulation s >= 1 goes to the best-scoring edge among those that hold the visit count the
            // sequential-halving schedule asks for; below the root the descent is the PUCT of the loop below, without noise,
            // or the interior rule (hive_search_set_gumbel_interior)
            float gum[4], logit[4], qhat[4], sigma[4];
            int nv[4], max_n, sum_n;
            wave_gumbel_root(S, g, eb, ne, root_turn, S.root_v[g], !quiet, lane, gum, logit, qhat, sigma, nv, max_n, sum_n);
            const int n_sched = (S.budget != nullptr ? S.budget[g] : S.gum.sims) - 1;
            const int m_eff = S.gum.max_considered < ne ? S.gum.max_considered : ne;
            const int t = gumbel_considered_visit(m_eff, n_sched, (int)sim - 1);
            float all = -3.0e38f;
            int aidx = 0x7FFFFFFF;
            for (int k = 0; k < 4; ++k)
                if (nv[k] >= 0) {
                    const float b = gumbel_score(gum[k], logit[k], sigma[k]);
                    if (b > all) { all = b; aidx = lane + 64 * k; }
                    if (nv[k] == t && b > best) { best = b; bidx = lane + 64 * k; }
                }
            wave_argmax(best, bidx);
            if (bidx == 0x7FFFFFFF) {                        // no edge holds that count (a root visit was taken back): all edges
                wave_argmax(all, aidx);
                bidx = aidx;
                if (lane == 0) S.gum_fallback[g] += 1;
            }
            if (bidx >= ne) bidx = 0;                        // (scores that are not numbers compare false everywhere)
        } else if (interior) {
            // Gumbel below the root: the edge whose visit share lags softmax(logit + sigma(completed q)) most; no noise, no
            // c_puct.  One slot only, so N holds no visit in flight but this descent's own (a line back into a node).
            bidx = 0;                                        // a single edge (the pass edge: P = 0) is taken as it is
            if (ne > 1) {
                float gum[4], logit[4], qhat[4], sigma[4], improved[4];
                int nv[4], max_n, sum_n;
                wave_gumbel_root(S, g, eb, ne, root_turn, S.node_v[nbase + node], false, lane, gum, logit, qhat, sigma, nv, max_n,
                                 sum_n);
                wave_gumbel_improved(logit, sigma, nv, improved);
                bidx = 0x7FFFFFFF;
                for (int k = 0; k < 4; ++k)
                    if (nv[k] >= 0) {
                        const float b = gumbel_interior_score(improved[k], nv[k], sum_n);
                        if (b > best) { best = b; bidx = lane + 64 * k; }
                    }
                wave_argmax(best, bidx);
                if (bidx >= ne) bidx = 0;                    // (scores that are not numbers compare false everywhere)
            }
        } else {
            for (int k = 0; k < 4; ++k) {
                int e = lane + 64 * k;
                if (e < ne && !((banned >> k) & 1u)) {
                    float p = S.e_p[eb + e], w = S.e_w[eb + e];
                    int n = S.e_n[eb + e];
                    float b;
                    if (uct) {
                        b = uct_score(w, (float)n, p, xx);
                    } else {
                        float q = n > 0 ? w / (float)n : 0.f;
                        if (noisy) p = (1.0f - S.prm.noise_eps) * p + S.prm.noise_eps * noise[k];
                        b = q + S.prm.c_puct * p * xx / (1.0f + (float)n);
                    }
                    if (b > best) { best = b; bidx = e; }
                }
            }
            wave_argmax(best, bidx);
        }
        int child = S.e_child[eb + bidx];
        if (child == -1 && S.n_nodes[g] + S.L >= S.MN) child = -2;    // node pool exhausted: treat as a collision
        if (lane == 0) {
            // virtual loss (solo_play.py:205-208)
            S.node_sum_n[nbase + node] += 1;
            S.e_n[eb + bidx] += 1;
            S.e_w[eb + bidx] -= S.prm.virtual_loss;
            pnode[depth] = node;
            pedge[depth] = bidx;
            apply_action(reinterpret_cast<HiveBoard *>(st), reinterpret_cast<HiveHistory *>(st + 16), S.e_act[eb + bidx]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        depth++;
        if (child == -1 && S.merge) {
            // `state in self.tree` (solo_play.py:188): the position may already have a node, reached by another move order
            const int known = tt_find(S, g, st, lane);
            if (known >= 0) {
                child = known;
                if (lane == 0) { S.e_child[eb + bidx] = known; S.tt_hits[g] += 1; }
            }
        }
        if (child == -1) {
            if (lane == 0) S.e_child[eb + bidx] = -2;                 // expansion in flight
            kind = LEAF_EXPAND; leafnode = node; leafedge = bidx;
            break;
        }
        if (child == -2 || depth >= S.MN - 1) { kind = LEAF_COLLISION; break; }
        node = child;
    }
    if (kind == LEAF_EXPAND) {
        wave_copy(&leaf_boards[g], st, sizeof(HiveBoard), lane);
        wave_copy(&leaf_hist[g], st + 16, sizeof(HiveHistory), lane);
    }
    if (lane == 0) {
        S.leaf_kind[sg] = (int8_t)kind;
        S.leaf_node[sg] = leafnode;
        S.leaf_edge[sg] = leafedge;
        S.path_len[sg] = depth;
    }
}

// expansion (solo_play.py:188-197,304-313) + backup (solo_play.py:217-247)
__global__ void __launch_bounds__(256)
search_backup_kernel(SearchDev S, int slot, const HiveBoard *__restrict__ leaf_boards,
                     const HiveHistory *__restrict__ leaf_hist, const uint32_t *__restrict__ leaf_mask,
                     const int8_t *__restrict__ over, const int8_t *__restrict__ winner, const float *__restrict__ p,
                     const float *__restrict__ v)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S.G) return;
    const long long sg = (long long)slot * S.G + g;
    const int kind = S.leaf_kind[sg];
    if (kind == LEAF_NONE) return;
    const long long nbase = (long long)g * S.MN;
    const int32_t *pnode = S.path_node + sg * S.MN, *pedge = S.path_edge + sg * S.MN;
    const int plen = S.path_len[sg];

    if (kind == LEAF_COLLISION) {
        // two in-flight selections met: take the virtual loss back, nothing to learn
        if (lane == 0)
            for (int d = 0; d < plen; ++d) {
                long long eb = (nbase + pnode[d]) * EC + pedge[d];
                S.node_sum_n[nbase + pnode[d]] -= 1;
                S.e_n[eb] -= 1;
                S.e_w[eb] += S.prm.virtual_loss;
            }
        if (lane == 0) S.kind_hist[g * 8 + LEAF_COLLISION] += 1;
        return;
    }
    const bool uct = S.prm.mode == HIVE_SEARCH_UCT;

    float ret;
    int known = -1;
    const bool capped = kind == LEAF_CAPDRAW ||
                        (kind == LEAF_EXPAND && !over[g] && (int)leaf_boards[g].turn >= S.prm.max_game_length);
    int stat = kind;                                        // hive_search_leaf_histogram bucket
    if (kind == LEAF_EXPAND && !capped && S.merge)          // another in-flight slot may have created this position meanwhile
        known = tt_find(S, g, reinterpret_cast<const uint32_t *>(&leaf_boards[g]), lane);
    const bool solver = solver_game(S, g);
    int proven = 0;                                         // status of the node where the path ended (wave-uniform)
    if (kind == LEAF_TERMINAL) {
        ret = S.node_tv[nbase + S.leaf_node[sg]];
        if (solver) proven = S.node_status[nbase + S.leaf_node[sg]];
    } else if (kind == LEAF_PROVEN) {
        // the descent stopped at a proven node: a known finished game, |status| - 1 plies early
        proven = S.node_status[nbase + S.leaf_node[sg]];
        ret = proven > 0 ? 1.0f : -1.0f;
        stat = LEAF_TERMINAL;
        if (lane == 0) S.solver_stats[g * 4 + 0] += 1;
    } else if (capped) {
        // length cap (solo_play.py:181-183): a property of this path's turn count, not of the position -- no node
        if (kind == LEAF_EXPAND && lane == 0) S.e_child[(nbase + S.leaf_node[sg]) * EC + S.leaf_edge[sg]] = -1;
        ret = uct ? 0.f : kDrawSentinel;                    // (UCT has no cap; 250 plies only guard the 8-bit turn counter)
        if (kind == LEAF_EXPAND) stat = 6;
    } else if (known >= 0) {
        if (lane == 0) S.e_child[(nbase + S.leaf_node[sg]) * EC + S.leaf_edge[sg]] = known;
        ret = S.node_term[nbase + known] ? S.node_tv[nbase + known] : v[g];
        if (solver) proven = S.node_status[nbase + known];
        stat = 7;
    } else {
        const int id = (kind == LEAF_ROOT) ? 0 : S.n_nodes[g];
        wave_copy(&S.node_board[nbase + id], &leaf_boards[g], sizeof(HiveBoard), lane);
        wave_copy(&S.node_hist[nbase + id], &leaf_hist[g], sizeof(HiveHistory), lane);
        if (S.merge) tt_insert(S, g, reinterpret_cast<const uint32_t *>(&leaf_boards[g]), id, lane);
        const unsigned turn = leaf_boards[g].turn;
        const int stm = (turn & 1u) ? 0 : 1;
        bool term = false;
        float tv = 0.f;
        int fresh = 0;                                      // the new node's status
        if (over[g] && uct) {
            // MCTS_chess.py:144-146: a finished game is never expanded; every visit backs up the network's value of
            // that same position -- the evaluator is a pure function of the planes, so the value is kept with the node
            term = true;
            tv = v[g];
        } else if (over[g]) {                               // solo_play.py:169-180
            term = true;
            int w = winner[g];
            tv = (w == 0) ? kDrawSentinel : ((w - 1) == stm ? 1.0f : -1.0f);
            fresh = (w == 0) ? 0 : ((w - 1) == stm ? 1 : -1);   // only a finished game with a winner proves anything
            stat = 6;
        } else if ((int)turn >= S.prm.max_game_length) {    // solo_play.py:181-183
            term = true;
            tv = kDrawSentinel;
        }
        const long long eb = (nbase + id) * EC;
        int ne = 0;
        if (!term) {
            // the leaf's legal set arrives as 11 destination boards (hive_abi.h); lane l of pass t owns action 64 t + l,
            // so the ballots below are the id-ordered mask words and the edges come out in ascending action order
            const uint32_t *m = leaf_mask + (long long)g * HIVE_MASK_WORDS;
            const float *pg = p + (long long)g * HIVE_ACTIONS;
            unsigned legal_bits = 0u;                       // bit t: action 64 t + lane is legal
            float tot = 0.f;
            for (int t = 0; t < 25; ++t) {
                const int a = t * 64 + lane;
                if (a < HIVE_ACTIONS && HIVE_MASK_TEST(m, a)) { legal_bits |= 1u << t; tot += pg[a]; }
            }
            tot = wave_sum(tot) + 1e-8f;                    // solo_play.py:305-312
            const float inv = uct ? 1.0f : 1.0f / tot;      // MCTS_chess.py:89-94: illegal priors zeroed, no renormalisation
            int total = 0;
            for (int t = 0; t < 25; ++t) {
                const bool mine = (legal_bits >> t) & 1u;
                const unsigned long long w = __ballot(mine);
                if (mine) {
                    int pos = total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(w >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)w, 0u));
                    if (pos < EC) {
                        int a = t * 64 + lane;
                        S.e_act[eb + pos] = (int16_t)a;
                        S.e_p[eb + pos] = pg[a] * inv;
                        S.e_n[eb + pos] = 0;
                        S.e_w[eb + pos] = 0.f;
                        S.e_child[eb + pos] = -1;
                        if (S.e_status != nullptr) S.e_status[eb + pos] = 0;
                    }
                }
                total += __popcll(w);
            }
            ne = total < EC ? total : EC;
            if (ne == 0 && uct) {
                // MCTS_chess.py:87-88: is_expanded stays False, the node is evaluated again on every visit (same value)
                term = true;
                tv = v[g];
            } else if (ne == 0) {                           // no legal move: the pass edge (solo_play.py:299-300)
                if (lane == 0) {
                    S.e_act[eb] = -1; S.e_p[eb] = 0.f; S.e_n[eb] = 0; S.e_w[eb] = 0.f; S.e_child[eb] = -1;
                    if (S.e_status != nullptr) S.e_status[eb] = 0;
                }
                ne = 1;
            }
        }
        if (lane == 0) {
            if (kind == LEAF_ROOT) S.root_v[g] = v[g];          // the Gumbel root completes unvisited edges with it
            S.node_nedge[nbase + id] = ne;
            S.node_sum_n[nbase + id] = 0;
            S.node_term[nbase + id] = term ? 1 : 0;
            S.node_tv[nbase + id] = tv;
            S.node_v[nbase + id] = term ? tv : v[g];            // the interior Gumbel rule completes unvisited edges with it
            if (S.node_status != nullptr) S.node_status[nbase + id] = (int8_t)fresh;
            S.n_nodes[g] = id + 1;
            if (kind == LEAF_EXPAND) S.e_child[(nbase + S.leaf_node[sg]) * EC + S.leaf_edge[sg]] = id;
        }
        ret = term ? tv : v[g];
        if (solver) proven = fresh;
    }
    if (lane == 0) {
        S.kind_hist[g * 8 + stat] += 1;
        const float vl = S.prm.virtual_loss;
        if (uct) {
            // MCTS_chess.py:111-119: every node from the leaf up to the root gets number_visits += 1 (done at selection)
            // and total_value += v if black is to move AT that node, -v if white is -- i.e. the edge leaving a position
            // with white to move (odd turn) collects +v
            for (int d = plen - 1; d >= 0; --d) {
                const long long eidx = (nbase + pnode[d]) * EC + pedge[d];
                const float sv = (S.node_board[nbase + pnode[d]].turn & 1u) ? ret : -ret;
                S.e_w[eidx] = vl != 0.f ? S.e_w[eidx] + (vl + sv) : S.e_w[eidx] + sv;
            }
        } else {
            float val = ret;
            for (int d = plen - 1; d >= 0; --d) {
                long long eidx = (nbase + pnode[d]) * EC + pedge[d];
                bool reach_max = (val == kDrawSentinel);    // solo_play.py:219-223
                float leaf_v = reach_max ? -1.0f : -val;
                S.e_w[eidx] += vl + leaf_v;                 // virtual_loss + leaf_v; n and sum_n: -vl + 1 = 0
                val = reach_max ? kDrawSentinel : leaf_v;   // solo_play.py:244-247
            }
        }
    }
    // proven results travel up this path (include/hive_search.h): the whole wave walks it, four edges per lane and a ballot
    // decide a node.  Backups run slot after slot, so no other wave writes this game's statuses meanwhile.
    int c = proven;
    for (int d = plen - 1; d >= 0 && c != 0 && c > -127 && c < 127; --d) {
        const int P = pnode[d], k = pedge[d];
        const long long eb = (nbase + P) * EC;
        const int own = c > 0 ? -(c + 1) : 1 - c;           // -sign(c) (|c| + 1)
        const int s = wave_solver_node_status(S.e_status + eb, S.node_nedge[nbase + P], k, own, lane);
        if (lane == 0) {
            const int old = S.node_status[nbase + P];
            S.e_status[eb + k] = (int8_t)own;
            S.node_status[nbase + P] = (int8_t)s;
            if (old == 0 && s > 0) S.solver_stats[g * 4 + 1] += 1;
            if (old == 0 && s < 0) S.solver_stats[g * 4 + 2] += 1;
        }
        wave_sync();                                         // a path may pass through P again further up
        c = s;
    }
}

// solo_play.py:337-374 + self_play.py:139-157
__global__ void __launch_bounds__(256)
search_policy_kernel(SearchDev S, const int8_t *__restrict__ which, float *__restrict__ policy, int32_t *__restrict__ action,
                     int32_t *__restrict__ sum_n_out, int selfplay)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S.G) return;
    float *pol = policy ? policy + (long long)g * HIVE_ACTIONS : nullptr;
    if (pol) for (int i = lane; i < HIVE_ACTIONS; i += 64) pol[i] = 0.f;
    // hive_search_policy_where: a game outside `which` is answered as an inactive one
    if ((which != nullptr && which[g] == 0) || !S.active[g] || S.n_nodes[g] == 0 || S.node_term[(long long)g * S.MN]) {
        if (lane == 0) { action[g] = -2; if (sum_n_out) sum_n_out[g] = 0; }
        return;
    }
    const long long nbase = (long long)g * S.MN, eb = nbase * EC;
    const int ne = S.node_nedge[nbase];
    if (gumbel_game(S, g)) {
        // Gumbel root: the move is the best-scoring edge among the most visited, the policy is softmax(logit + sigma(completed
        // q)) over every edge.  Neither the "every W negative" fallback nor the opening resampling applies.
        const bool quiet = S.quiet != nullptr && S.quiet[g] != 0;
        float gum[4], logit[4], qhat[4], sigma[4], improved[4];
        int nv[4], max_n, visits;
        wave_gumbel_root(S, g, eb, ne, S.node_board[nbase].turn, S.root_v[g], !quiet, lane, gum, logit, qhat, sigma, nv, max_n,
                         visits);
        wave_gumbel_improved(logit, sigma, nv, improved);
        float best = -3.0e38f;
        int bidx = 0x7FFFFFFF;
        for (int k = 0; k < 4; ++k)
            if (nv[k] >= 0) {
                const int e = lane + 64 * k, a = S.e_act[eb + e];
                if (pol && a >= 0) pol[a] = improved[k];
                const float b = gumbel_score(gum[k], logit[k], sigma[k]);
                if (nv[k] == max_n && b > best) { best = b; bidx = e; }
            }
        wave_argmax(best, bidx);
        if (bidx >= ne) bidx = 0;                               // (scores that are not numbers compare false everywhere)
        if (lane == 0) {
            action[g] = S.e_act[eb + bidx];
            if (sum_n_out) sum_n_out[g] = visits;
        }
        return;
    }
    int nsum = 0;
    float wmax = -3.0e38f;
    for (int k = 0; k < 4; ++k) {
        int e = lane + 64 * k;
        if (e < ne) { nsum += S.e_n[eb + e]; wmax = fmaxf(wmax, S.e_w[eb + e]); }
    }
    nsum = wave_sum_i(nsum);
    wmax = wave_max(wmax);
    // solo_play.py:372-373 (HivePlayer falls back to the priors when every W is negative); MCTS_chess.py:157-161
    // (get_policy) has no such rule -- before the first backed-up visit its policy is all zero
    const bool uct = S.prm.mode == HIVE_SEARCH_UCT;
    const bool use_prior = uct ? false : ((wmax < 0.f) || nsum == 0);
    const unsigned turn = S.node_board[nbase].turn;
    // proven wins and losses (include/hive_search.h): a root whose status holds answers from the proof; otherwise the
    // moves proven to lose leave the choice below -- never the policy row -- unless every move is one
    unsigned banned = 0u;                                   // bit k: edge lane + 64 k is a proven loss that holds
    int from_proof = -1;
    if (solver_game(S, g)) {
        const int cap = S.prm.max_game_length, s0 = S.node_status[nbase];
        const bool root_holds = solver_holds(s0, (int)turn, cap);
        const int8_t *es = S.e_status + eb;
        long long key = -1;                                 // (speed of the proof, visits, lower edge first), larger is better
        bool open = false;
        for (int k = 0; k < 4; ++k) {
            const int e = lane + 64 * k;
            if (e < ne) {
                const int x = es[e];
                const bool holds = solver_holds(x, (int)turn, cap);
                if (x < 0 && holds) banned |= 1u << k;
                else open = true;
                if (root_holds && holds && (s0 > 0) == (x > 0)) {
                    const long long speed = s0 > 0 ? 128 - x : -x;
                    const long long kk = (speed << 40) | ((long long)S.e_n[eb + e] << 8) | (long long)(255 - e);
                    key = kk > key ? kk : key;
                }
            }
        }
        if (__ballot(open) == 0ull) banned = 0u;
        for (int o = 32; o > 0; o >>= 1) { const long long x = __shfl_xor(key, o); key = x > key ? x : key; }
        if (root_holds && key >= 0) from_proof = 255 - (int)(key & 255);
    }
    float pi[4];
    float best = -1.f;
    int bidx = 0x7FFFFFFF;
    for (int k = 0; k < 4; ++k) {
        int e = lane + 64 * k;
        pi[k] = 0.f;
        if (e < ne) {
            pi[k] = use_prior ? S.e_p[eb + e] : (nsum > 0 ? (float)S.e_n[eb + e] / (float)nsum : 0.f);
            int a = S.e_act[eb + e];
            if (pol && a >= 0) pol[a] = pi[k];
            if (((banned >> k) & 1u) == 0u && pi[k] > best) { best = pi[k]; bidx = e; }
        }
    }
    wave_argmax(best, bidx);                                // tau < 0.1 always => argmax (solo_play.py:338-345)
    int chosen = bidx;
    if (from_proof >= 0) {
        if (lane == 0) {
            action[g] = S.e_act[eb + from_proof];
            if (sum_n_out) sum_n_out[g] = nsum;
            S.solver_stats[g * 4 + 3] += 1;
        }
        return;
    }
    if (selfplay && S.e_act[eb] >= 0) {
        // self_play.py:143-157: e = 0.7 - int(turn+1)/2 * 0.15; resample while e >= 0.1 (turns 1..6)
        float err = 0.7f - 0.5f * (float)(turn + 1u) * 0.15f;
        if (turn <= 6u) {
            float nz[4], tot = 0.f;
            for (int k = 0; k < 4; ++k) {
                int e = lane + 64 * k;
                nz[k] = 0.f;
                if (e < ne) {
                    Rng r = noise_rng(S.seed ^ 0xD1B54A32D192ED03ull, S.game_id[g], turn, 0ull, 0, e);
                    nz[k] = r.gamma(0.5f);
                    tot += nz[k];
                }
            }
            tot = wave_sum(tot);
            float inv = tot > 0.f ? 1.0f / tot : 0.f, psum = 0.f;
            for (int k = 0; k < 4; ++k) {
                nz[k] = (1.0f - err) * pi[k] + err * nz[k] * inv;
                if ((banned >> k) & 1u) nz[k] = 0.f;        // a move proven to lose is not drawn
                psum += nz[k];
            }
            psum = wave_sum(psum);
            Rng r = noise_rng(S.seed ^ 0xA24BAED4963EE407ull, S.game_id[g], turn, 0ull, 0, 7777);
            float target = r.uniform() * psum;
            // inclusive prefix over edges in index order: lanes hold e = lane + 64k, so scan k-major
            float acc = 0.f;
            int pick = ne - 1;
            bool done = false;
            for (int k = 0; k < 4 && !done; ++k) {
                float x = nz[k], incl = x;
                for (int o = 1; o < 64; o <<= 1) {
                    float y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                float row_total = __shfl(incl, 63);
                bool hit = (lane + 64 * k < ne) && (acc + incl >= target);
                unsigned long long hm = __ballot(hit);
                if (hm) { pick = 64 * k + (int)__builtin_ctzll(hm); done = true; }
                acc += row_total;
            }
            chosen = pick;
        }
    }
    if (lane == 0) {
        action[g] = S.e_act[eb + chosen];
        if (sum_n_out) sum_n_out[g] = nsum;
    }
}

// hive_search_leaf_need: which of the selected leaves will search_backup_kernel ask the network about?  Exactly the
// conditions of that kernel: a finished game (PUCT), a leaf at the length cap, a revisited terminal node, a collision and an
// idle tree take their value from elsewhere -- the evaluator may skip their rows.
__global__ void __launch_bounds__(256)
search_need_kernel(SearchDev S, int slots, const HiveBoard *__restrict__ leaf_boards, const int8_t *__restrict__ over,
                   int8_t *__restrict__ need, unsigned long long *__restrict__ total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)slots * S.G;
    bool want = false;
    if (i < n) {
        const int kind = S.leaf_kind[i];
        want = kind == LEAF_ROOT || kind == LEAF_EXPAND;
        if (want && S.prm.mode != HIVE_SEARCH_UCT)
            want = !over[i] && (int)leaf_boards[i].turn < S.prm.max_game_length;
        need[i] = want ? 1 : 0;
    }
    if (total) {
        const unsigned long long w = __ballot(want);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(total, (unsigned long long)__popcll(w));
    }
}

// UCTNode.child_number_visits / child_total_value / child_priors of the root (MCTS_chess.py:33-35) as dense action-indexed rows
__global__ void __launch_bounds__(256)
search_root_stats_kernel(SearchDev S, float *__restrict__ visits, float *__restrict__ total_value, float *__restrict__ priors)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S.G) return;
    const long long row = (long long)g * HIVE_ACTIONS;
    for (int i = lane; i < HIVE_ACTIONS; i += 64) {
        if (visits) visits[row + i] = 0.f;
        if (total_value) total_value[row + i] = 0.f;
        if (priors) priors[row + i] = 0.f;
    }
    if (!S.active[g] || S.n_nodes[g] == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const long long eb = (long long)g * S.MN * EC;
    const int ne = S.node_term[(long long)g * S.MN] ? 0 : S.node_nedge[(long long)g * S.MN];
    for (int e = lane; e < ne; e += 64) {
        const int a = S.e_act[eb + e];
        if (a < 0) continue;
        if (visits) visits[row + a] = (float)S.e_n[eb + e];
        if (total_value) total_value[row + a] = S.e_w[eb + e];
        if (priors) priors[row + a] = S.e_p[eb + e];
    }
}

// hive_search_root_status: one thread per game
__global__ void __launch_bounds__(256)
search_root_status_kernel(SearchDev S, int8_t *__restrict__ status)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.G) return;
    const bool tree = S.node_status != nullptr && S.active[g] && S.n_nodes[g] > 0;
    status[g] = tree ? S.node_status[(long long)g * S.MN] : (int8_t)0;
}

// hive_search_sample_noise: one wave per draw, the same wave_dirichlet / mixing arithmetic as search_select_kernel
__global__ void __launch_bounds__(256)
search_noise_kernel(unsigned long long seed, long long first_game, unsigned turn, float alpha, int k, int draws,
                    const float *__restrict__ prior, float eps, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= draws) return;
    float noise[4];
    wave_dirichlet(noise, k, alpha, seed, first_game + d, turn, 0ull, 0, lane);
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        if (e < k) out[(long long)d * k + e] = prior ? (1.0f - eps) * prior[e] + eps * noise[j] : noise[j];
    }
}

// hive_search_gumbel_schedule: the device's schedule function, entry by entry
__global__ void __launch_bounds__(256)
search_gumbel_schedule_kernel(int m, int n, int32_t *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gumbel_considered_visit(m, n, i);
}

// hive_search_root_gumbel: the per-edge quantities of every root as search_select_kernel / search_policy_kernel see them
// now, in edge order; zero rows for a game without a tree, zeros past the last edge
__global__ void __launch_bounds__(256)
search_root_gumbel_kernel(SearchDev S, float *__restrict__ gum_out, float *__restrict__ logit_out, float *__restrict__ qhat_out,
                          float *__restrict__ improved_out)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S.G) return;
    const long long nbase = (long long)g * S.MN, eb = nbase * EC, row = (long long)g * EC;
    const bool tree = S.active[g] && S.n_nodes[g] > 0 && !S.node_term[nbase];
    const int ne = tree ? (S.node_nedge[nbase] < EC ? S.node_nedge[nbase] : EC) : 0;
    float gum[4], logit[4], qhat[4], sigma[4], improved[4];
    int nv[4] = {-1, -1, -1, -1}, max_n, visits;
    if (tree) {
        const bool quiet = S.quiet != nullptr && S.quiet[g] != 0;
        wave_gumbel_root(S, g, eb, ne, S.node_board[nbase].turn, S.root_v[g], !quiet, lane, gum, logit, qhat, sigma, nv, max_n,
                         visits);
        wave_gumbel_improved(logit, sigma, nv, improved);
    }
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        const bool on = nv[k] >= 0;
        if (gum_out) gum_out[row + e] = on ? gum[k] : 0.f;
        if (logit_out) logit_out[row + e] = on ? logit[k] : 0.f;
        if (qhat_out) qhat_out[row + e] = on ? qhat[k] : 0.f;
        if (improved_out) improved_out[row + e] = on ? improved[k] : 0.f;
    }
}

// hive_search_draw_budgets: one thread per game.  Full or fast ply: a pure function of (seed, game id, root turn) -- the
// first output of the generator keyed like every other draw here, on a stream constant of its own
constexpr unsigned long long kBudgetStream = 0x8CB92BA72F3D8DD7ull;
__global__ void __launch_bounds__(256)
search_draw_budgets_kernel(unsigned long long seed, const long long *__restrict__ game_id, const HiveBoard *__restrict__ roots,
                           const int8_t *__restrict__ active, int n, int full_sims, int fast_sims, uint32_t full_threshold,
                           int32_t *__restrict__ budget, int8_t *__restrict__ quiet, int8_t *__restrict__ full)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const bool on = active ? active[g] != 0 : true;
    const unsigned long long x = splitmix(Rng(seed ^ kBudgetStream, (unsigned long long)game_id[g],
                                              (unsigned long long)roots[g].turn, 0ull).s);
    // a saturated threshold (p_full = 1) is "always"
    const bool f = on && (full_threshold == 0xFFFFFFFFu || (uint32_t)(x >> 32) < full_threshold);
    budget[g] = on ? (f ? full_sims : fast_sims) : 0;
    if (quiet) quiet[g] = (on && !f) ? 1 : 0;
    if (full) full[g] = f ? 1 : 0;
}

// hive_search_round_end: one thread per game, after the backups of a rolling round
__global__ void __launch_bounds__(256)
search_round_end_kernel(SearchDev S, int slots_run, int8_t *__restrict__ done)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.G) return;
    const bool on = S.active[g] != 0;
    const int b = S.budget[g];
    int c = S.clock[g];
    if (on && c < b) {
        const int left = b - c;
        c += c == 0 ? 1 : (slots_run < left ? slots_run : left);      // the root-opening simulation runs alone
        S.clock[g] = c;
    }
    done[g] = (on && c >= b) ? 1 : 0;
}

// hive_search_advance_roots: the subtree under the played root edge becomes the tree of the next search.  One wave per
// game; LDS per wave: map[MN] (old node -> new index, -1 = not reached) and queue[MN] (breadth-first order = the new
// numbering).  The kept nodes are written into the second pool D; the host swaps the pools after the launch.  Every
// loop is bounded by MN (a node enters the queue once), 64 (lanes of a ballot) or TT.
__global__ void __launch_bounds__(256)
search_advance_kernel(SearchDev S, NodePool D, const int32_t *__restrict__ played, const HiveBoard *__restrict__ boards,
                      const HiveHistory *__restrict__ hist, const int8_t *__restrict__ active)
{
    extern __shared__ int32_t advance_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * (int)(blockDim.x >> 6) + wv;
    if (g >= S.G) return;
    int32_t *map = advance_lds + (long long)wv * 2 * S.MN, *queue = map + S.MN;
    const long long nbase = (long long)g * S.MN;
    const bool act = active ? active[g] != 0 : true;
    const int n_old = S.n_nodes[g] < S.MN ? S.n_nodes[g] : S.MN;
    const int pl = played ? played[g] : -3;

    // what search_reset_kernel does, for every game
    wave_copy(&S.root_board[g], &boards[g], sizeof(HiveBoard), lane);
    wave_copy(&S.root_hist[g], &hist[g], sizeof(HiveHistory), lane);
    for (int i = lane; i < S.TT; i += 64) S.tt[(long long)g * S.TT + i] = -1;

    // the child under the played edge: expanded, not a finished game, and really the caller's position
    int c = -1;
    if (act && pl >= -1 && n_old > 0 && !S.node_term[nbase]) {
        const int ne = S.node_nedge[nbase] < EC ? S.node_nedge[nbase] : EC;
        int edge = -1;
        for (int k = 0; k < 4 && edge < 0; ++k) {
            const int e = lane + 64 * k;
            const unsigned long long m = __ballot(e < ne && (int)S.e_act[nbase * EC + e] == pl);
            if (m) edge = 64 * k + (int)__builtin_ctzll(m);
        }
        if (edge >= 0) {
            const int ch = S.e_child[nbase * EC + edge];
            if (ch >= 0 && ch < n_old && !S.node_term[nbase + ch] &&
                key_equal(reinterpret_cast<const uint32_t *>(&S.node_board[nbase + ch]),
                          reinterpret_cast<const uint32_t *>(&boards[g]), lane))
                c = ch;
        }
    }

    int kept = 0, visits = 0;
    if (c >= 0) {
        // closure of c under e_child >= 0: the transposition table makes the tree a graph with cycles, so nodes are marked
        for (int i = lane; i < S.MN; i += 64) map[i] = -1;
        wave_sync();
        if (lane == 0) { map[c] = 0; queue[0] = c; }
        wave_sync();
        kept = 1;
        for (int head = 0; head < kept && head < S.MN; ++head) {
            const int node = queue[head];
            const int ne = S.node_nedge[nbase + node] < EC ? S.node_nedge[nbase + node] : EC;
            const long long eb = (nbase + node) * EC;
            for (int k = 0; 64 * k < ne; ++k) {
                const int e = lane + 64 * k;
                int ch = e < ne ? S.e_child[eb + e] : -1;
                if (ch >= n_old) ch = -1;
                bool want = ch >= 0 && map[ch] < 0;
                unsigned long long m = __ballot(want);
                while (m) {                                  // new children in edge order; two edges into one child count once
                    const int nc = __shfl(ch, (int)__builtin_ctzll(m));
                    if (lane == 0 && kept < S.MN) { map[nc] = kept; queue[kept] = nc; }
                    kept++;
                    if (ch == nc) want = false;
                    m = __ballot(want);
                }
                wave_sync();
            }
        }
        if (kept > S.MN) kept = S.MN;                        // (cannot happen: at most n_old <= MN distinct nodes)
        visits = S.node_sum_n[nbase + c];
        if (kept + S.sims_room > S.MN) {                     // no room left for the next search: start fresh, and say so
            if (lane == 0) S.carry_refused[g] += 1;
            c = -1;
        }
    }
    if (c < 0) {
        if (lane == 0) {
            S.n_nodes[g] = 0;
            S.root_pending[g] = 0;
            S.active[g] = act ? 1 : 0;
            S.carry_kept[g] = 0;
            S.carry_visits[g] = 0;
        }
        return;
    }

    for (int i = 0; i < kept; ++i) {
        const long long so = nbase + queue[i], dn = nbase + i;
        // node 0 takes the caller's records: the key holds neither the turn number nor the history, and the simulation's
        // env is staged from node 0
        wave_copy(&D.node_board[dn], i == 0 ? &boards[g] : &S.node_board[so], sizeof(HiveBoard), lane);
        wave_copy(&D.node_hist[dn], i == 0 ? &hist[g] : &S.node_hist[so], sizeof(HiveHistory), lane);
        const int ne = S.node_nedge[so] < EC ? S.node_nedge[so] : EC;
        if (lane == 0) {
            D.node_nedge[dn] = S.node_nedge[so];
            D.node_sum_n[dn] = S.node_sum_n[so];
            D.node_term[dn] = S.node_term[so];
            D.node_tv[dn] = S.node_tv[so];
            D.node_v[dn] = S.node_v[so];
            if (S.node_status != nullptr) D.node_status[dn] = S.node_status[so];
        }
        for (int e = lane; e < ne; e += 64) {
            if (S.e_status != nullptr) D.e_status[dn * EC + e] = S.e_status[so * EC + e];
            D.e_act[dn * EC + e] = S.e_act[so * EC + e];
            D.e_p[dn * EC + e] = S.e_p[so * EC + e];
            D.e_n[dn * EC + e] = S.e_n[so * EC + e];
            D.e_w[dn * EC + e] = S.e_w[so * EC + e];
            const int ch = S.e_child[so * EC + e];
            D.e_child[dn * EC + e] = (ch >= 0 && ch < n_old) ? map[ch] : -1;      // (-2 = in flight: none between searches)
        }
    }
    if (S.merge) {
        wave_sync();                                         // the cleared table
        const uint32_t mask = (uint32_t)S.TT - 1u;
        for (int i = 0; i < kept; ++i) {
            const HiveBoard *rec = i == 0 ? &boards[g] : &S.node_board[nbase + queue[i]];
            uint32_t slot = key_hash(reinterpret_cast<const uint32_t *>(rec), lane) & mask;
            if (lane == 0)                                   // one lane probes and writes: its loads follow its own stores
                for (int probe = 0; probe < S.TT; ++probe, slot = (slot + 1u) & mask)
                    if (S.tt[(long long)g * S.TT + slot] < 0) { S.tt[(long long)g * S.TT + slot] = i; break; }
        }
    }
    if (lane == 0) {
        S.n_nodes[g] = kept;
        S.root_pending[g] = 0;
        S.active[g] = 1;
        S.carry_kept[g] = kept;
        S.carry_visits[g] = visits;
    }
}

}  // namespace hive

// ====================================================================== host side / C ABI
using namespace hive;

extern "C" const char *hive_last_error(void);
namespace hive { int set_error(int code, const std::string &msg); }

#define S_TRY(expr)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return hive::set_error(HIVE_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct HiveSearch {
    SearchDev d{};
    int device = 0;
    hipStream_t stream = nullptr;
    unsigned long long sim = 0;
    void *pool[72];
    int npool = 0;
    NodePool alt{};             // second node pool of hive_search_advance_roots, allocated on first use
    bool have_alt = false;
    int32_t *clock_mem = nullptr;   // hive_search_set_rolling: the per-game clocks, allocated on first use
};

template <typename T>
static hipError_t alloc(HiveSearch *s, T **p, size_t count)
{
    hipError_t e = hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * count);
    if (e == hipSuccess) s->pool[s->npool++] = *p;
    return e;
}

extern "C" {

static int search_alloc(HiveSearch *s, int games, int max_nodes, int slots)
{
    SearchDev &d = s->d;
    const size_t GN = (size_t)games * max_nodes, GE = GN * EC, LG = (size_t)slots * games;
    S_TRY(alloc(s, &d.node_board, GN));
    S_TRY(alloc(s, &d.node_hist, GN));
    S_TRY(alloc(s, &d.node_nedge, GN));
    S_TRY(alloc(s, &d.node_sum_n, GN));
    S_TRY(alloc(s, &d.node_term, GN));
    S_TRY(alloc(s, &d.node_tv, GN));
    S_TRY(alloc(s, &d.node_v, GN));
    S_TRY(alloc(s, &d.e_act, GE));
    S_TRY(alloc(s, &d.e_p, GE));
    S_TRY(alloc(s, &d.e_w, GE));
    S_TRY(alloc(s, &d.e_n, GE));
    S_TRY(alloc(s, &d.e_child, GE));
    S_TRY(alloc(s, &d.n_nodes, (size_t)games));
    S_TRY(alloc(s, &d.active, (size_t)games));
    S_TRY(alloc(s, &d.root_pending, (size_t)games));
    S_TRY(alloc(s, &d.root_board, (size_t)games));
    S_TRY(alloc(s, &d.root_hist, (size_t)games));
    S_TRY(alloc(s, &d.path_node, LG * max_nodes));
    S_TRY(alloc(s, &d.path_edge, LG * max_nodes));
    S_TRY(alloc(s, &d.path_len, LG));
    S_TRY(alloc(s, &d.leaf_kind, LG));
    S_TRY(alloc(s, &d.leaf_node, LG));
    S_TRY(alloc(s, &d.leaf_edge, LG));
    d.TT = 64;
    while (d.TT < 2 * max_nodes) d.TT *= 2;
    d.merge = 1;
    S_TRY(alloc(s, &d.tt, (size_t)games * d.TT));
    S_TRY(alloc(s, &d.tt_hits, (size_t)games));
    S_TRY(alloc(s, &d.game_id, (size_t)games));
    S_TRY(alloc(s, &d.kind_hist, (size_t)games * 8));
    S_TRY(hipMemset(d.kind_hist, 0, sizeof(int32_t) * (size_t)games * 8));
    S_TRY(alloc(s, &d.carry_kept, (size_t)games));
    S_TRY(alloc(s, &d.carry_visits, (size_t)games));
    S_TRY(alloc(s, &d.carry_refused, (size_t)games));
    S_TRY(hipMemset(d.carry_kept, 0, sizeof(int32_t) * (size_t)games));
    S_TRY(hipMemset(d.carry_visits, 0, sizeof(int32_t) * (size_t)games));
    S_TRY(hipMemset(d.carry_refused, 0, sizeof(int32_t) * (size_t)games));
    S_TRY(alloc(s, &d.root_v, (size_t)games));
    S_TRY(alloc(s, &d.gum_fallback, (size_t)games));
    S_TRY(hipMemset(d.root_v, 0, sizeof(float) * (size_t)games));
    S_TRY(hipMemset(d.gum_fallback, 0, sizeof(int32_t) * (size_t)games));
    S_TRY(alloc(s, &d.solver_stats, (size_t)games * 4));
    S_TRY(hipMemset(d.solver_stats, 0, sizeof(int32_t) * (size_t)games * 4));
    {
        long long *ids = new (std::nothrow) long long[games];
        if (ids == nullptr) return hive::set_error(HIVE_E_DEVICE, "hive_search_create: out of host memory");
        for (int i = 0; i < games; ++i) ids[i] = i;
        hipError_t e = hipMemcpy(d.game_id, ids, sizeof(long long) * (size_t)games, hipMemcpyHostToDevice);
        delete[] ids;
        S_TRY(e);
    }
    S_TRY(hipMemset(d.tt, 0xFF, sizeof(int32_t) * (size_t)games * d.TT));
    S_TRY(hipMemset(d.tt_hits, 0, sizeof(int32_t) * games));
    S_TRY(hipMemset(d.n_nodes, 0, sizeof(int32_t) * games));
    S_TRY(hipMemset(d.active, 0, games));
    S_TRY(hipMemset(d.root_pending, 0, games));
    S_TRY(hipMemset(d.leaf_kind, 0, LG));
    S_TRY(hipMemset(d.path_len, 0, sizeof(int32_t) * LG));
    S_TRY(hipMemset(d.node_term, 0, GN));
    S_TRY(hipMemset(d.node_v, 0, sizeof(float) * GN));
    return HIVE_OK;
}

int hive_search_destroy(HiveSearch *s);

int hive_search_create(int games, int max_nodes, int slots, int device, uint64_t seed, HiveSearch **out)
{
    if (games <= 0 || max_nodes < 2 || slots < 1 || slots > HIVE_MAX_SLOTS || !out)
        return hive::set_error(HIVE_E_ARG, "hive_search_create: bad argument");
    *out = nullptr;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        return hive::set_error(HIVE_E_DEVICE, "hive_search_create: no HIP device visible (no CPU path)");
    if (device < 0 || device >= cnt) return hive::set_error(HIVE_E_ARG, "hive_search_create: bad device ordinal");
    S_TRY(hipSetDevice(device));
    HiveSearch *s = new (std::nothrow) HiveSearch();
    if (s == nullptr) return hive::set_error(HIVE_E_DEVICE, "hive_search_create: out of host memory");
    s->device = device;
    s->d.G = games; s->d.MN = max_nodes; s->d.L = slots; s->d.seed = seed;
    s->d.sims_room = slots + 2;
    s->d.prm = HiveSearchParams{0.7f, 0.25f, 0.3f, 55, HIVE_SEARCH_PUCT, 1.0f};
    int rc = search_alloc(s, games, max_nodes, slots);
    if (rc != HIVE_OK) {            // free whatever was allocated; the caller never sees a partial handle
        hive_search_destroy(s);
        return rc;
    }
    *out = s;
    return HIVE_OK;
}

int hive_search_destroy(HiveSearch *s)
{
    if (!s) return HIVE_OK;
    (void)hipSetDevice(s->device);
    for (int i = 0; i < s->npool; ++i) (void)hipFree(s->pool[i]);
    delete s;
    return HIVE_OK;
}

int hive_search_set_stream(HiveSearch *s, void *stream)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    s->stream = (hipStream_t)stream;
    return HIVE_OK;
}

int hive_search_set_params(HiveSearch *s, const HiveSearchParams *p)
{
    if (!s || !p) return hive::set_error(HIVE_E_ARG, "null argument");
    if ((p->mode != HIVE_SEARCH_PUCT && p->mode != HIVE_SEARCH_UCT) || !(p->virtual_loss >= 0.f) || p->max_game_length < 1 ||
        p->max_game_length > 250)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_params: unknown mode, negative virtual loss or length cap outside 1..250");
    if (s->d.gum_on && p->mode == HIVE_SEARCH_UCT)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_params: the Gumbel root is on and has no UCT form (hive_search_set_gumbel)");
    if (s->d.solver_on && p->mode == HIVE_SEARCH_UCT)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_params: proven results are on and have no UCT form (hive_search_set_solver)");
    s->d.prm = *p;
    return HIVE_OK;
}

static dim3 wave_grid(int games) { return dim3((unsigned)((games + 3) / 4)); }

int hive_search_set_roots(HiveSearch *s, const HiveBoard *boards, const HiveHistory *hist, const int8_t *active)
{
    if (!s || !boards || !hist) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_reset_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, (const int8_t *)nullptr, boards,
                       hist, active);
    S_TRY(hipGetLastError());
    s->sim = 0;                 // simulations are numbered inside one search: part of the noise key (hive_search_set_game_ids)
    return HIVE_OK;
}

int hive_search_set_rolling(HiveSearch *s, int on)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    S_TRY(hipSetDevice(s->device));
    if (!on) {
        s->d.clock = nullptr;
        return HIVE_OK;
    }
    if (s->clock_mem == nullptr) S_TRY(alloc(s, &s->clock_mem, (size_t)s->d.G));
    S_TRY(hipMemsetAsync(s->clock_mem, 0, sizeof(int32_t) * (size_t)s->d.G, s->stream));
    s->d.clock = s->clock_mem;
    return HIVE_OK;
}

int hive_search_restart(HiveSearch *s, const int8_t *which, const HiveBoard *boards, const HiveHistory *hist,
                        const int8_t *active)
{
    if (!s || !which || !boards || !hist) return hive::set_error(HIVE_E_ARG, "null argument");
    if (!s->d.clock) return hive::set_error(HIVE_E_ARG, "hive_search_restart: the handle is not rolling (hive_search_set_rolling)");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_reset_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, which, boards, hist, active);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_round_end(HiveSearch *s, int slots_run, int8_t *done)
{
    if (!s || !done || slots_run < 1 || slots_run > s->d.L) return hive::set_error(HIVE_E_ARG, "hive_search_round_end: bad argument");
    if (!s->d.clock || !s->d.budget)
        return hive::set_error(HIVE_E_ARG, "hive_search_round_end: needs hive_search_set_rolling and hive_search_set_budgets");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_round_end_kernel, dim3((unsigned)((s->d.G + 255) / 256)), dim3(256), 0, s->stream, s->d, slots_run,
                       done);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_clocks(HiveSearch *s, int32_t *clock)
{
    if (!s || !clock) return hive::set_error(HIVE_E_ARG, "null argument");
    if (!s->d.clock) return hive::set_error(HIVE_E_ARG, "hive_search_clocks: the handle is not rolling (hive_search_set_rolling)");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(clock, s->d.clock, sizeof(int32_t) * (size_t)s->d.G, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_set_budgets(HiveSearch *s, const int32_t *budget, const int8_t *quiet)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    if (!budget && quiet) return hive::set_error(HIVE_E_ARG, "hive_search_set_budgets: quiet without budget");
    s->d.budget = budget;
    s->d.quiet = quiet;
    return HIVE_OK;
}

int hive_search_set_gumbel(HiveSearch *s, const HiveGumbelParams *prm, const int8_t *where)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    if (!prm) {
        s->d.gum_on = 0;
        s->d.gum_where = nullptr;
        return HIVE_OK;
    }
    if (s->d.prm.mode == HIVE_SEARCH_UCT)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_gumbel: the Gumbel root has no UCT form (PUCT mode only)");
    if (s->d.solver_on)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_gumbel: not with proven results (hive_search_set_solver): a proven root "
                                           "ends descents at depth 0 and the halving schedule counts root visits");
    if (s->d.L > 1)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_gumbel: one slot only -- visits in flight would desynchronise the "
                                           "sequential-halving schedule");
    if (prm->max_considered < 1 || !(prm->c_visit >= 0.f) || !(prm->c_scale > 0.f) || prm->sims < 1)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_gumbel: max_considered and sims must be at least 1, c_visit >= 0, "
                                           "c_scale > 0");
    s->d.gum = *prm;
    s->d.gum_where = where;
    s->d.gum_on = 1;
    return HIVE_OK;
}

int hive_search_set_gumbel_interior(HiveSearch *s, int on, const int8_t *where)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    // read by Gumbel games alone (gumbel_game): accepted before or after hive_search_set_gumbel, in any mode
    s->d.gum_int_on = on ? 1 : 0;
    s->d.gum_int_where = on ? where : nullptr;
    return HIVE_OK;
}

int hive_search_set_solver(HiveSearch *s, int on, const int8_t *where)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    if (!on) {
        s->d.solver_on = 0;
        s->d.solver_where = nullptr;
        return HIVE_OK;
    }
    if (s->d.prm.mode == HIVE_SEARCH_UCT)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_solver: proven results have no UCT form (PUCT mode only)");
    if (s->d.gum_on)
        return hive::set_error(HIVE_E_ARG, "hive_search_set_solver: not with the Gumbel root (hive_search_set_gumbel): its halving "
                                           "schedule counts root visits and a proven root ends descents at depth 0");
    S_TRY(hipSetDevice(s->device));
    if (s->d.node_status == nullptr) {
        // both pools at once: hive_search_advance_roots moves the statuses with the nodes, whichever call came first
        const size_t GN = (size_t)s->d.G * s->d.MN, GE = GN * EC;
        int8_t *ns[2] = {nullptr, nullptr}, *es[2] = {nullptr, nullptr};
        for (int i = 0; i < 2; ++i) {
            S_TRY(alloc(s, &ns[i], GN));
            S_TRY(alloc(s, &es[i], GE));
            S_TRY(hipMemsetAsync(ns[i], 0, GN, s->stream));
            S_TRY(hipMemsetAsync(es[i], 0, GE, s->stream));
        }
        s->d.e_status = es[0];
        s->alt.e_status = es[1];
        s->alt.node_status = ns[1];
        s->d.node_status = ns[0];
    }
    s->d.solver_where = where;
    s->d.solver_on = 1;
    return HIVE_OK;
}

int hive_search_node_status(HiveSearch *s, int game, int8_t *node, int8_t *edge)
{
    if (!s || game < 0 || game >= s->d.G) return hive::set_error(HIVE_E_ARG, "hive_search_node_status: bad argument");
    S_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)s->d.MN, o = (size_t)game * N;
    if (s->d.node_status == nullptr) {
        if (node) S_TRY(hipMemsetAsync(node, 0, N, s->stream));
        if (edge) S_TRY(hipMemsetAsync(edge, 0, N * EC, s->stream));
        return HIVE_OK;
    }
    if (node) S_TRY(hipMemcpyAsync(node, s->d.node_status + o, N, hipMemcpyDeviceToDevice, s->stream));
    if (edge) S_TRY(hipMemcpyAsync(edge, s->d.e_status + o * EC, N * EC, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_root_status(HiveSearch *s, int8_t *status)
{
    if (!s || !status) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_root_status_kernel, dim3((unsigned)((s->d.G + 255) / 256)), dim3(256), 0, s->stream, s->d, status);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_solver_stats(HiveSearch *s, int32_t *out)
{
    if (!s || !out) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(out, s->d.solver_stats, sizeof(int32_t) * (size_t)s->d.G * 4, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_node_values(HiveSearch *s, int game, float *node_v)
{
    if (!s || !node_v || game < 0 || game >= s->d.G) return hive::set_error(HIVE_E_ARG, "hive_search_node_values: bad argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(node_v, s->d.node_v + (size_t)game * s->d.MN, sizeof(float) * (size_t)s->d.MN, hipMemcpyDeviceToDevice,
                         s->stream));
    return HIVE_OK;
}

int hive_search_gumbel_schedule(int m, int n, int32_t *out_dev, void *stream)
{
    if (m < 1 || n < 1 || !out_dev) return hive::set_error(HIVE_E_ARG, "hive_search_gumbel_schedule: bad argument");
    hipLaunchKernelGGL(search_gumbel_schedule_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, n,
                       out_dev);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_root_gumbel(HiveSearch *s, float *g, float *logit, float *qhat, float *improved)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    if (!s->d.gum_on) return hive::set_error(HIVE_E_ARG, "hive_search_root_gumbel: the Gumbel root is off (hive_search_set_gumbel)");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_root_gumbel_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, g, logit, qhat, improved);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_gumbel_fallbacks(HiveSearch *s, int32_t *count)
{
    if (!s || !count) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(count, s->d.gum_fallback, sizeof(int32_t) * (size_t)s->d.G, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_draw_budgets(uint64_t seed, const int64_t *game_id, const HiveBoard *root_boards, const int8_t *active, int n,
                             int full_sims, int fast_sims, uint32_t full_threshold, int32_t *budget, int8_t *quiet, int8_t *full,
                             void *stream)
{
    if (!game_id || !root_boards || !budget || n <= 0 || full_sims < 0 || fast_sims < 0)
        return hive::set_error(HIVE_E_ARG, "hive_search_draw_budgets: bad argument");
    hipLaunchKernelGGL(search_draw_budgets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)seed, reinterpret_cast<const long long *>(game_id), root_boards, active, n, full_sims,
                       fast_sims, full_threshold, budget, quiet, full);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_set_carry_room(HiveSearch *s, int sims_room)
{
    if (!s || sims_room < 0) return hive::set_error(HIVE_E_ARG, "hive_search_set_carry_room: bad argument");
    s->d.sims_room = sims_room;
    return HIVE_OK;
}

int hive_search_advance_roots(HiveSearch *s, const int32_t *played, const HiveBoard *boards, const HiveHistory *hist,
                              const int8_t *active)
{
    if (!s || !boards || !hist) return hive::set_error(HIVE_E_ARG, "null argument");
    if (s->d.clock)
        return hive::set_error(HIVE_E_ARG, "hive_search_advance_roots: not with per-game clocks (hive_search_set_rolling)");
    if (s->d.gum_on)
        return hive::set_error(HIVE_E_ARG, "hive_search_advance_roots: not with the Gumbel root (hive_search_set_gumbel): a carried "
                                           "root has no network value and no fresh schedule");
    S_TRY(hipSetDevice(s->device));
    SearchDev &d = s->d;
    // LDS per game: map + queue, 8 bytes per node; four games per workgroup while that fits into 64 KB, else one
    const size_t per_wave = sizeof(int32_t) * 2 * (size_t)d.MN;
    const int waves = 4 * per_wave <= 65536 ? 4 : 1;
    if (per_wave > 65536)
        return hive::set_error(HIVE_E_ARG, "hive_search_advance_roots: max_nodes above 8192 does not fit the LDS reach mask");
    if (!s->have_alt) {
        const size_t GN = (size_t)d.G * d.MN, GE = GN * EC;
        NodePool &a = s->alt;
        S_TRY(alloc(s, &a.node_board, GN));
        S_TRY(alloc(s, &a.node_hist, GN));
        S_TRY(alloc(s, &a.node_nedge, GN));
        S_TRY(alloc(s, &a.node_sum_n, GN));
        S_TRY(alloc(s, &a.node_term, GN));
        S_TRY(alloc(s, &a.node_tv, GN));
        S_TRY(alloc(s, &a.node_v, GN));
        S_TRY(alloc(s, &a.e_act, GE));
        S_TRY(alloc(s, &a.e_p, GE));
        S_TRY(alloc(s, &a.e_w, GE));
        S_TRY(alloc(s, &a.e_n, GE));
        S_TRY(alloc(s, &a.e_child, GE));
        S_TRY(hipMemset(a.node_term, 0, GN));
        S_TRY(hipMemset(a.node_v, 0, sizeof(float) * GN));
        s->have_alt = true;
    }
    hipLaunchKernelGGL(search_advance_kernel, dim3((unsigned)((d.G + waves - 1) / waves)), dim3(64 * waves), waves * per_wave,
                       s->stream, d, s->alt, played, boards, hist, active);
    S_TRY(hipGetLastError());
    // every later launch (stream order) works on the pool the kernel wrote
    const NodePool old{d.node_board, d.node_hist, d.node_nedge, d.node_sum_n, d.node_term, d.node_tv, d.node_v,
                       d.e_act, d.e_p, d.e_w, d.e_n, d.e_child, d.node_status, d.e_status};
    const NodePool &a = s->alt;
    d.node_board = a.node_board; d.node_hist = a.node_hist; d.node_nedge = a.node_nedge; d.node_sum_n = a.node_sum_n;
    d.node_term = a.node_term; d.node_tv = a.node_tv; d.node_v = a.node_v; d.e_act = a.e_act; d.e_p = a.e_p; d.e_w = a.e_w;
    d.e_n = a.e_n; d.e_child = a.e_child; d.node_status = a.node_status; d.e_status = a.e_status;
    s->alt = old;
    s->sim = 0;
    return HIVE_OK;
}

int hive_search_carry_stats(HiveSearch *s, int32_t *kept_nodes, int32_t *carried_visits, int32_t *refused)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    S_TRY(hipSetDevice(s->device));
    const size_t bytes = sizeof(int32_t) * (size_t)s->d.G;
    if (kept_nodes) S_TRY(hipMemcpyAsync(kept_nodes, s->d.carry_kept, bytes, hipMemcpyDeviceToDevice, s->stream));
    if (carried_visits) S_TRY(hipMemcpyAsync(carried_visits, s->d.carry_visits, bytes, hipMemcpyDeviceToDevice, s->stream));
    if (refused) S_TRY(hipMemcpyAsync(refused, s->d.carry_refused, bytes, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_export_tree(HiveSearch *s, int game, int32_t *n_nodes, HiveBoard *boards, HiveHistory *hist, int32_t *nedge,
                            int32_t *sum_n, int8_t *term, float *tv, int16_t *e_act, float *e_p, int32_t *e_n, float *e_w,
                            int32_t *e_child)
{
    if (!s || game < 0 || game >= s->d.G) return hive::set_error(HIVE_E_ARG, "hive_search_export_tree: bad argument");
    S_TRY(hipSetDevice(s->device));
    const SearchDev &d = s->d;
    const size_t N = (size_t)d.MN, o = (size_t)game * N;
#define EXPORT_COPY(dst, src, count)                                                                                    \
    if (dst) S_TRY(hipMemcpyAsync(dst, src, sizeof(*(dst)) * (count), hipMemcpyDeviceToDevice, s->stream))
    EXPORT_COPY(n_nodes, d.n_nodes + game, 1);
    EXPORT_COPY(boards, d.node_board + o, N);
    EXPORT_COPY(hist, d.node_hist + o, N);
    EXPORT_COPY(nedge, d.node_nedge + o, N);
    EXPORT_COPY(sum_n, d.node_sum_n + o, N);
    EXPORT_COPY(term, d.node_term + o, N);
    EXPORT_COPY(tv, d.node_tv + o, N);
    EXPORT_COPY(e_act, d.e_act + o * EC, N * EC);
    EXPORT_COPY(e_p, d.e_p + o * EC, N * EC);
    EXPORT_COPY(e_n, d.e_n + o * EC, N * EC);
    EXPORT_COPY(e_w, d.e_w + o * EC, N * EC);
    EXPORT_COPY(e_child, d.e_child + o * EC, N * EC);
#undef EXPORT_COPY
    return HIVE_OK;
}

int hive_search_select(HiveSearch *s, int slot, HiveBoard *leaf_boards, HiveHistory *leaf_hist)
{
    if (!s || !leaf_boards || !leaf_hist || slot < 0 || slot >= s->d.L) return hive::set_error(HIVE_E_ARG, "bad argument");
    if (s->d.clock && !s->d.budget)
        return hive::set_error(HIVE_E_ARG, "hive_search_select: per-game clocks need budgets (hive_search_set_budgets)");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_select_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, slot, s->sim++, leaf_boards,
                       leaf_hist);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_backup(HiveSearch *s, int slot, const HiveBoard *leaf_boards, const HiveHistory *leaf_hist,
                       const uint32_t *leaf_mask, const int8_t *over, const int8_t *winner, const float *p, const float *v)
{
    if (!s || !leaf_boards || !leaf_hist || !leaf_mask || !over || !winner || !p || !v || slot < 0 || slot >= s->d.L)
        return hive::set_error(HIVE_E_ARG, "bad argument");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_backup_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, slot, leaf_boards, leaf_hist,
                       leaf_mask, over, winner, p, v);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_leaf_need(HiveSearch *s, int slots, const HiveBoard *leaf_boards, const int8_t *over, int8_t *need,
                          uint64_t *total)
{
    if (!s || !leaf_boards || !over || !need || slots < 1 || slots > s->d.L) return hive::set_error(HIVE_E_ARG, "bad argument");
    S_TRY(hipSetDevice(s->device));
    const long long n = (long long)slots * s->d.G;
    hipLaunchKernelGGL(search_need_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->d, slots, leaf_boards,
                       over, need, reinterpret_cast<unsigned long long *>(total));
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_policy(HiveSearch *s, float *policy, int32_t *action, int32_t *sum_n, int selfplay)
{
    if (!s || !action) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_policy_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, (const int8_t *)nullptr, policy,
                       action, sum_n, selfplay);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_policy_where(HiveSearch *s, const int8_t *which, float *policy, int32_t *action, int32_t *sum_n, int selfplay)
{
    if (!s || !which || !action) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_policy_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, which, policy, action, sum_n,
                       selfplay);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_set_transpositions(HiveSearch *s, int merge)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    s->d.merge = merge ? 1 : 0;
    return HIVE_OK;
}

int hive_search_transposition_hits(HiveSearch *s, int32_t *hits)
{
    if (!s || !hits) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(hits, s->d.tt_hits, sizeof(int32_t) * s->d.G, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_node_counts(HiveSearch *s, int32_t *counts)
{
    if (!s || !counts) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(counts, s->d.n_nodes, sizeof(int32_t) * s->d.G, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_set_game_ids(HiveSearch *s, const int64_t *ids)
{
    if (!s || !ids) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(s->d.game_id, ids, sizeof(long long) * (size_t)s->d.G, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_root_stats(HiveSearch *s, float *visits, float *total_value, float *priors)
{
    if (!s) return hive::set_error(HIVE_E_ARG, "null handle");
    S_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(search_root_stats_kernel, wave_grid(s->d.G), dim3(256), 0, s->stream, s->d, visits, total_value, priors);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

int hive_search_leaf_histogram(HiveSearch *s, int32_t *hist)
{
    if (!s || !hist) return hive::set_error(HIVE_E_ARG, "null argument");
    S_TRY(hipSetDevice(s->device));
    S_TRY(hipMemcpyAsync(hist, s->d.kind_hist, sizeof(int32_t) * (size_t)s->d.G * 8, hipMemcpyDeviceToDevice, s->stream));
    return HIVE_OK;
}

int hive_search_sample_noise(uint64_t seed, int64_t first_game, int turn, float alpha, int k, int draws, const float *prior,
                             float eps, float *out, void *stream)
{
    if (!out || k < 1 || k > HIVE_EDGE_CAP || draws < 1 || !(alpha > 0.f) || turn < 0 || turn > 255)
        return hive::set_error(HIVE_E_ARG, "hive_search_sample_noise: bad argument");
    hipLaunchKernelGGL(search_noise_kernel, wave_grid(draws), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (long long)first_game, (unsigned)turn, alpha, k, draws, prior, eps, out);
    S_TRY(hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
